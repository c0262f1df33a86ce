// kernels_tail.hpp -- the long tail of tiny rounds inside ONE persistent workgroup.
//
// At the BASELINE sizes > 98 % of all rounds have <= 64 bidders and
// every round depends on the prices of the previous one, so the tail is a latency chain, not a
// bandwidth problem.  One workgroup (one CU) loops over rounds on the
// device: the unassigned list lives in LDS, bids are formed per person (auction_.pyx:339-365),
// conflicts are resolved in LDS (:375-385), winners are applied (:388-427) and the list is
// compacted (push_all_left, :137-162) without leaving the kernel.  K never grows inside an
// eps-phase (every winner evicts at most one owner), so once K <= threshold the whole rest of the
// phase runs here.  The kernels exit when K == 0 or nits == max_iter.
//
// A bid is first tried on the person's CANDIDATE LINE (device_common.hpp: 256 bytes, <= 30 price records, an
// exactness test) and only on a miss by a full scan of the row, which also rebuilds the line.  With the lines -- and
// k_bid refreshing the nearly spent ones in the grid rounds -- 99 % of the tail's bids need one 256-byte read and one
// 30-wide record gather instead of the whole row and ~200 gathers; the dependent chain of a round is
// line -> records -> 32-lane reduction -> next line.
//
// A round is a serial chain of dependent instructions per wavefront, so what makes it shorter is wavefronts: one
// kernel per role (at the end of this file; a mode is a function above them), launched back to back once per phase (K
// only falls), each with the registers and the LDS of its role alone -- all roles in one kernel: 185 VGPRs, spills:
//   k_tail_block (K > 16;  1024 threads): two list slots per wavefront and sweep (one per 32-lane half, one gather
//         serves both), misses queued and scanned in a second pass; a clean round (no object bid on twice, none unowned:
//         the test runs in front of the barrier) is finished by the threads = slots, any other by wavefront 0 (LDS hash
//         table above 64 bidders);
//   k_tail_team (3 <= K <= 16; 1024 threads): wavefront w serves slot w alone; ONE LDS-only barrier per round, every
//         serving wavefront finishes the round for the whole list on lanes = slots;
//   k_tail_pair (K <= 2; 64 threads): one wavefront, no barrier, no LDS but the two list slots; K = 2: both bidders'
//         lines in the two 32-lane halves, one evaluation for both (tail_pair_mode); K = 1: the chain;
//   k_tail_nolines (512 threads), for a handle whose lines are switched off, behind k_tail_block: every mode (team
//         mode with two slots per wavefront, solo mode -- the older form of the pair round -- for K = 2).
// Both edge layouts keep lines; in the 12 B/edge layout a slot's cost comes from a parallel line of fp64 costs
// (device_common.hpp: Slot64).
//
// Visibility: records / lines are written and re-read by this one workgroup only (same CU, same
// vector L1, barriers between phases); the CSR is read-only.  No other workgroup runs.
#pragma once
#include "device_common.hpp"

namespace misslap {

struct TailArgs {
    Ctl *ctl;
    const int *row_ptr;
    double *price;
    PriceRec *rec;  // {price, owner, owner's row start} per object, see device_common.hpp
    int *p2o;
    int *o2p;
    int *U;
    int2 *cand;     // candidate lines (nullptr: none)
    double *cand64; // ... their fp64 costs (12 B/edge layout only, nullptr otherwise)
    int thr;
    int round_budget;  // > 0: a kernel returns to the host after so many rounds (the host then refreshes the
                       // lines of long rows, which the kernels cannot rebuild in place, and launches again); 0 = no limit
    float eps;
};

constexpr int kHashSize = 2048;  // LDS open-addressing table for K > 64 (load factor <= 0.5)

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
    const int lo = __builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffull), l);
    const int hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}

// assignment of one winner (auction_.pyx:396-418); returns the new content of its U slot.  Inside the tail
// kernel the price record is the ONLY copy that is kept current: one 16-byte store per winner instead of
// five scattered ones, and price[] / o2p[] / p2o[] lines stay out of the CU's L2 working set.  k_sync_from_rec
// rebuilds the three plain arrays from the records when the kernel has finished.
__device__ __forceinline__ int apply_winner(const TailArgs &a, int person, int pstart, int obj, int prev,
                                            unsigned long long key) {
    PriceRec r;
    r.price = key_to_bid(key);
    r.owner = person;
    r.ostart = pstart;
    a.rec[obj] = r;
    return prev;  // evicted owner inherits the slot (:409); -1 = hole (:412)
}

// After the tail kernels: price[j], o2p[j] from the records, and p2o as the inverse of o2p.  p2o needs no clearing pass:
// every person is either the owner of exactly one record (written below) or unassigned, and the unassigned persons are
// the list U[0, K) -- K <= the tail threshold of them.
struct k_sync_from_rec {
    MISSLAP_KERNEL(256)
    static __device__ __forceinline__ void run(Ctl *ctl, const PriceRec *rec, double *price, int *o2p, int *p2o, const int *U, int n_cols, int lines, unsigned long long *live, unsigned ticket) {
        const int K = ctl->K;
        // (closes a run of tail kernels: K / nits are theirs; an error bit raised below reaches the host with the next status)
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            post_live_status(live, ticket, K, ctl->err, ctl->nits);
            ctl->n_need = 0;  // the maintenance pass's work list has been consumed
        }
        for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < K; n += gridDim.x * blockDim.x) {
            const int i = U[n];
            if (i >= 0) p2o[i] = -1;
        }
        for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n_cols; j += gridDim.x * blockDim.x) {
            const PriceRec r = rec[j];
            // price[] still holds the prices the tail kernels started from: a price may only have risen since (the
            // candidate lines rely on it; a net fall means eps is below the rounding error of a price update).  A handle
            // WITHOUT lines does not depend on the invariant -- there a falling price is what the reference computes too
            if (lines && r.price < price[j]) atomicOr(&ctl->err, kErrPriceFell);
            price[j] = r.price;
            o2p[j] = r.owner;
            if (r.owner >= 0) p2o[r.owner] = j;
        }
    }
};


// per-wavefront statistics, flushed once when the kernel ends
// (what can be derived is not counted in the rounds: line hits = bids - misses, their edges = edges - miss_edges)
struct TailStats {
    unsigned long long edges, miss_edges, builds;
    unsigned bids, misses;
    unsigned bad_hi;  // largest high word of a bid made from a line, per LANE (cand_eval1_lane; bad_hi_is_error)
    int err;
    double hint;  // cand_build's search distance, carried from one build of this wavefront to the next
};

// zero in every lane, but not wave-uniform to the compiler: an index built with it goes through the VECTOR memory
// path.  A wave-uniform row_ptr[person + 1] would be a scalar load, which shares lgkmcnt with LDS and makes every
// LDS-only barrier wait an L2 / HBM latency for a value nobody needs yet.
__device__ __forceinline__ int lane_zero() {
    return (int)__builtin_amdgcn_mbcnt_hi(0u, __builtin_amdgcn_mbcnt_lo(0u, 0u));
}

// What a wavefront requests for its (up to) two persons ahead of their bids: the candidate lines -- person A's in
// lanes 0..31, person B's in lanes 32..63, they answer ~90 % of the bids -- and, speculatively, the first 256 edges of
// both rows plus the row ends, so that a miss costs one memory latency, not two.  The lines are requested FIRST: a
// wavefront's loads return in issue order, so a line can be used while the rows are still on their way, and a hit
// never waits for a row at all.
// the lane's slot of a line that never hits: tau = +inf in slot 0, every other slot empty
template <class Slot>
__device__ __forceinline__ Slot cand_no_line() {
    return (lane_id() & (kCandLanes - 1)) == 0 ? LineIO<Slot>::make(0, 0x7ff00000) : LineIO<Slot>::make(-1, 0);
}
// the lane's slot of person `p`'s line (l32 = lane & 31)
template <class E>
__device__ __forceinline__ typename E::Slot line_of(const TailArgs &a, int p, int l32) {
    return LineIO<typename E::Slot>::load(a.cand, a.cand64, (size_t)max(p, 0) * kCandLanes + l32);
}
template <class E>
struct TwoFetch {
    typename E::Slot slot;      // the lane's slot of its half's line
    typename E::Raw row[2][4];  // 12 B/edge layout (no lines): first four 64-edge chunks of each row, requested ahead
    int ev[2];                  // ... and the row ends (vector registers, the same value in every lane)
};
template <class E>
__device__ __forceinline__ void fetch_row(const TailArgs &a, const E &ed, int person, int start,
                                          typename E::Raw (&row)[4], int &e) {
    const int lane = lane_id();
#pragma unroll
    for (int u = 0; u < 4; ++u) row[u] = ed.load_raw_nt(start + u * kWave + lane);  // the edge arrays are padded
    e = a.row_ptr[max(person, 0) + 1 + lane_zero()];
}
// Request what the next bids of persons p0 / p1 (-1 = none: a valid, unused address is read) need first: with
// candidate lines the two lines (p0's in lanes 0..31, p1's in lanes 32..63); without (12 B/edge layout) the rows.
// A wavefront's loads return in issue order, so nothing is requested speculatively BEHIND which a later,
// more urgent load would have to wait: rows are only read when a line has not decided.
template <class E>
__device__ __forceinline__ void request_two(const TailArgs &a, const E &ed, int p0, int s0, int p1, int s1,
                                            TwoFetch<E> &tf) {
    if (E::kCand) {
        const int pme = lane_id() < kCandLanes ? p0 : p1;
        tf.slot = a.cand != nullptr ? line_of<E>(a, pme, lane_id() & (kCandLanes - 1)) : cand_no_line<typename E::Slot>();
    } else {
        fetch_row<E>(a, ed, p0, s0, tf.row[0], tf.ev[0]);
        fetch_row<E>(a, ed, p1, s1, tf.row[1], tf.ev[1]);
    }
}

__device__ __forceinline__ void tail_build(const TailArgs &a, int person, const CandBuildArgs &ba, double eps,
                                           TailStats &st) {
    cand_build(a.cand, a.cand64, person, ba, eps, st.hint);
    st.builds += 1;
}

// ---- the exact paths that several modes share; no clean round of any mode runs one of them ----------------------------
// (left as they are: bid_two's scan, which rebuilds the line of a first miss in front of a second, and the block round's
// push_all_left, which serves 64 slots through LDS)
// A line did not decide: the bid by a full scan of the person's row [start, row_end), counted as a miss.  `bd` is what
// the rebuild of the line needs (tail_build); when that runs is the caller's business.
template <class E>
__device__ __forceinline__ void tail_scan(const TailArgs &a, const E &ed, int start, int row_end, double eps, CandBid &b,
                                          CandBuildArgs &bd, TailStats &st) {
    const typename E::Raw none[4] = {};
    wave_bid_full<E, RecSource, true, false>(ed, RecSource{a.rec}, start, row_end, none, eps, b, bd, st.err);
    st.misses += 1;
    st.miss_edges += (unsigned long long)b.len;
}
// RESOLVE (:375-385) on lanes = slots, all pairs via readlane: true where the lane's bid loses its object (strict ">":
// the earlier list position keeps an object on equal bids)
__device__ __forceinline__ bool lanes_lose(int obj, unsigned long long key, int K, int lane) {
    bool lose = false;
    for (int m = 0; m < K; ++m) {
        const int om = __builtin_amdgcn_readlane(obj, m);
        const bool same = (om == obj) && (m != lane);
        if (__any(same)) {  // wave-uniform
            const unsigned long long km = readlane_u64(key, m);
            lose |= same && (km > key || (km == key && m < lane));
        }
    }
    return lose;
}
// push_all_left (:137-162) on lanes = slots, K <= 63: lane l holds slot l's person `u` (-1: a hole) and its row start;
// the k-th hole left of K' takes the k-th person right of it.  Returns K'.
__device__ __forceinline__ int lanes_push_left(int &u, int &sx, bool act, int K, int lane) {
    const unsigned long long kmask = (1ull << K) - 1ull;
    const unsigned long long holes = __ballot(act && u == -1) & kmask;
    const int Kn = K - __popcll(holes);
    const unsigned long long lmask = (1ull << Kn) - 1ull;
    unsigned long long hl = holes & lmask;            // empty slots left of K'
    unsigned long long mv = ~holes & ~lmask & kmask;  // persons right of K'
    while (hl) {  // wave-uniform
        const int hk = __ffsll((long long)hl) - 1, mk = __ffsll((long long)mv) - 1;
        const int mu = __builtin_amdgcn_readlane(u, mk), ms = __builtin_amdgcn_readlane(sx, mk);
        if (lane == hk) {
            u = mu;
            sx = ms;
        }
        hl &= hl - 1;
        mv &= mv - 1;
    }
    return Kn;
}
// RESOLVE (:375-385) on two slots that bid on ONE object: strict ">" -- the earlier list position keeps it on equal bids
__device__ __forceinline__ void two_resolve(unsigned long long key0, unsigned long long key1, bool &win0, bool &win1) {
    if (key1 > key0) win0 = false;
    else win1 = false;
}
// ... behind ASSIGN (:396-418): a winner's slot goes to the evicted owner (:409) or becomes a hole (:412), a loser
// stays; push_all_left (:137-162) on two slots.  Returns K.
__device__ __forceinline__ int two_pass_on(int (&pi)[2], int (&ps)[2], bool win0, bool win1, const int (&prev)[2],
                                           const int (&pst)[2]) {
    if (win0) pi[0] = prev[0], ps[0] = pst[0];
    if (win1) pi[1] = prev[1], ps[1] = pst[1];
    if (pi[0] == -1 && pi[1] != -1) pi[0] = pi[1], ps[0] = ps[1], pi[1] = -1;
    return (pi[0] != -1) + (pi[1] != -1);
}
// ... and, when a two-slot mode ends, the two slots go back to the list
__device__ __forceinline__ void two_hand_back(int *sU, int *sStart, const int (&pi)[2], const int (&ps)[2]) {
    if (lane_id() == 0) sU[0] = pi[0], sU[1] = pi[1], sStart[0] = ps[0], sStart[1] = ps[1];
}

// The bids of the wavefront's two persons (auction_.pyx:339-365): both lines by one gather, then a full scan for
// every person whose line did not decide.  `early(b)` is cand_eval2's hook (the winners' owners are known).  The
// rebuild of the (last) scanned person's line is left to the caller (bd / bd_person), who first publishes the bids
// and requests the next data.
template <class E, class Early, class S = NoStamp>
__device__ __forceinline__ void bid_two(const TailArgs &a, const E &ed, const int (&pi)[2], const int (&ps)[2],
                                        TwoFetch<E> &tf, double eps, CandBid (&b)[2], CandBuildArgs &bd,
                                        int &bd_person, TailStats &st, Early &&early, const S &stamp = S()) {
    const RecSource src{a.rec};
    b[0].hit = b[1].hit = false;
    if (E::kCand) cand_eval2(tf.slot, pi[0] >= 0, pi[1] >= 0, src, eps, b, st.err, early, stamp);
    stamp.light(4);  // lines evaluated
    bd_person = -1;
#pragma unroll
    for (int X = 0; X < 2; ++X) {
        if (pi[X] < 0) continue;  // wave-uniform
        if (!b[X].hit) {
            if (bd_person >= 0) tail_build(a, bd_person, bd, eps, st);  // two misses in one round: rare
            if (E::kCand) {
                const typename E::Raw none[4] = {};
                const int e = a.row_ptr[pi[X] + 1 + lane_zero()];
                wave_bid_full<E, RecSource, true, false>(ed, src, ps[X], e, none, eps, b[X], bd, st.err);
            } else {
                wave_bid_full<E, RecSource, true, true>(ed, src, ps[X], tf.ev[X], tf.row[X], eps, b[X], bd, st.err);
            }
            bd.want = bd.want && a.cand != nullptr;
            bd_person = bd.want ? pi[X] : -1;
            st.misses += 1;
            st.miss_edges += (unsigned long long)b[X].len;
        }
        st.edges += (unsigned long long)b[X].len;
        st.bids += 1;
    }
}

// rounds a mode may run, as 32 bits (a mode that stops short of K's range or max_iter is simply entered again: budgeted
// launches already work that way)
__device__ __forceinline__ int round_limit(long long nits, long long max_iter) {
    return (int)min(max_iter - nits, (long long)0x7fffffff);
}

// ---- chain mode: K == 1 --------------------------------------------------------------------------------------------
// One bidder per round until the phase ends (K never grows): the bidder always wins (:375-385 has nothing to
// resolve), the evicted owner inherits the only slot (:409) and bids next, and the chain ends when an unowned object
// is won.  The owner and its row start come with the winning price record, so the only dependent memory accesses of
// a round are the bidder's line and the records of its candidates; the next line is requested as soon as the winning
// candidate is known.  Everything a round does not need (second list slot, resolve, push_all_left) is left out: a
// round is bound by the length of its dependent instruction sequence.
template <class E>
__device__ __forceinline__ void tail_chain_mode(const TailArgs &a, const E &ed, int &pi, int &ps, int &K,
                                                long long &nits, const long long max_iter, const double eps,
                                                TailStats &st) {
    const int lane = lane_id(), l32 = lane & (kCandLanes - 1);
    const RecSource src{a.rec};
    const bool cls = (lane >= 1) & (lane <= kCandMax);
    const bool lines = E::kCand && a.cand != nullptr;
    typename E::Slot slot = cand_no_line<typename E::Slot>();
    typename E::Raw row[4];  // (no lines): the row, requested ahead
    int ev = 0;
    auto request = [&](int person, int start) {
        if (E::kCand) {
            if (lines) slot = line_of<E>(a, person, l32);
        } else {
            fetch_row<E>(a, ed, person, start, row, ev);
        }
    };
    request(pi, ps);
    const int rmax = round_limit(nits, max_iter);  // (rounds are counted in 32 bits inside a mode)
    int r = 0;
#ifdef MISSLAP_TAIL_STAMP
    // diagnostic build: cycles per segment of a chain round -> Ctl::dbg[6..11]: [6] wait for the line, [7] record
    // gather, [8] winner known + next line requested, [9] rest of the evaluation, [10] full scan of a missed person,
    // [11] store / re-request / line rebuild
    unsigned long long sacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sprev = __builtin_amdgcn_s_memtime();
    const CycleStamp stamp{sacc, &sprev, true};
#else
    const NoStamp stamp;
#endif
    for (;;) {
        LaneBid w = {};
        int sp = -2;  // the person whose line was requested early (-2: nothing requested)
        if (E::kCand) {
            stamp(1);  // (diagnostic builds: drains the memory counters) the line has landed
            const PriceRec g = cand_gather1(slot, cls, src);
            stamp(2);  // the records have landed
            cand_eval1_lane(slot, g, cls, eps, w, st.bad_hi, [&](int prev) {
                sp = prev;
                request(sp, 0);
            }, stamp);
        }
        stamp.light(4);
        // ASSIGN (:396-418) is one store by the lane that holds the winning candidate, from its own registers
        bool store = w.mine;
        double bid = w.bid;
        int obj = w.obj, len = w.len;
        int nprev = w.prev, npst = w.pstart;
        if (!w.hit) {  // wave-uniform (rare behind the maintenance pass: the scan and the line's rebuild stay inside this
                       // block -- what the rebuild needs must not be carried across the join with the common path); the
                       // scan's result is wave-uniform and lane 0 stores it
            CandBid b;
            CandBuildArgs bd;
            if (E::kCand) {
                tail_scan(a, ed, ps, a.row_ptr[pi + 1], eps, b, bd, st);
            } else {
                wave_bid_full<E, RecSource, true, true>(ed, src, ps, ev, row, eps, b, bd, st.err);
                st.misses += 1;
                st.miss_edges += (unsigned long long)b.len;
            }
            if (bd.want && lines) tail_build(a, pi, bd, eps, st);
            store = lane == 0;
            bid = key_to_bid(b.key);
            obj = b.obj;
            len = b.len;
            nprev = b.prev;
            npst = b.pstart;
        }
        stamp.light(5);
        st.edges += (unsigned long long)len;
        st.bids += 1;
        r += 1;
        if (store) {
            PriceRec n;
            n.price = bid;
            n.owner = pi;
            n.ostart = ps;
            a.rec[(unsigned)obj] = n;  // (an object: >= 0, no sign extension)
        }
        pi = nprev;  // the evicted owner inherits the slot (:409) and bids next; -1: everybody is assigned
        ps = npst;
        const bool done = pi < 0 || r >= rmax;
        if (!done && sp != pi) request(pi, ps);  // (a scanned row decided differently from its line)
        stamp.light(6);
        if (done) break;
    }
    K = pi != -1;
    nits += r;
#ifdef MISSLAP_TAIL_STAMP
    if (lane == 0) {
        for (int k = 1; k <= 6; ++k) a.ctl->dbg[5 + k] += sacc[k];
    }
#endif
}

// ---- solo mode: K <= 2 ---------------------------------------------------------------------------------------------
// Wavefront 0 runs the rounds alone until the phase ends (K never grows), without barriers and without LDS.  The
// reference's round is reproduced operation by operation: both bids use the prices of the previous round (records
// are stored after both bids are formed), RESOLVE keeps the earlier list position on equal bids (:379), the evicted
// owner inherits the winner's slot (:409), push_all_left moves slot 1 into an emptied slot 0 (:137-162).  The next
// bidder of a slot is the owner its bidder evicts, and that owner comes with the winning price record -- no o2p /
// row_ptr look-ups between rounds: its line is requested as soon as the winning candidate is known, before the
// second-best reduction, the bid, the resolve step and the record stores of the current round.  A line that had to
// be rebuilt is rebuilt after the next round's data has been requested.
template <class E>
__device__ __forceinline__ void tail_solo_mode(const TailArgs &a, const E &ed, int *sU, int *sStart, int &K,
                                               long long &nits, const long long max_iter, const double eps,
                                               TailStats &st) {
    const int lane = lane_id();
    int pi[2], ps[2];
    pi[0] = __builtin_amdgcn_readfirstlane(sU[0]);
    ps[0] = __builtin_amdgcn_readfirstlane(sStart[0]);
    pi[1] = K > 1 ? __builtin_amdgcn_readfirstlane(sU[1]) : -1;
    ps[1] = K > 1 ? __builtin_amdgcn_readfirstlane(sStart[1]) : 0;
    if (K == 1) {
        tail_chain_mode(a, ed, pi[0], ps[0], K, nits, max_iter, eps, st);
        two_hand_back(sU, sStart, pi, ps);
        return;
    }
    TwoFetch<E> tf;
    tf.slot = cand_no_line<typename E::Slot>();
    request_two(a, ed, pi[0], ps[0], pi[1], ps[1], tf);
#ifdef MISSLAP_TAIL_STAMP_SOLO
    // diagnostic build: cycles of wavefront 0 per segment of a solo round -> Ctl::dbg[6..11] (+ dbg[15] = rounds):
    // [6] wait for the line, [7] record gather, [8] winner known + next line requested, [9] rest of the line
    // evaluation, [10] full scans of missed persons, [11] resolve / stores / re-request / line rebuild
    unsigned long long sacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sprev = __builtin_amdgcn_s_memtime();
    const CycleStamp stamp{sacc, &sprev, true};
#else
    const NoStamp stamp;
#endif
    for (;;) {
        CandBid b[2];
        CandBuildArgs bd;
        int bd_person;
        int sp[2] = {-2, -2};  // persons whose lines were requested early (-2: nothing requested)
        bid_two(a, ed, pi, ps, tf, eps, b, bd, bd_person, st, [&](const CandBid(&w)[2]) {
            sp[0] = pi[0] >= 0 ? w[0].prev : -1;
            sp[1] = pi[1] >= 0 ? w[1].prev : -1;
            request_two(a, ed, sp[0], 0, sp[1], 0, tf);  // (kCand only: the row starts are not needed)
        }, stamp);
        stamp.light(5);  // full scans of missed persons done
        nits += 1;
        // RESOLVE (:375-385), ASSIGN (:396-418) by lane 0, then the slots pass on
        bool win0 = true, win1 = pi[1] >= 0;
        if (win1 && b[0].obj == b[1].obj) two_resolve(b[0].key, b[1].key, win0, win1);
        if (lane == 0) {
            if (win0) apply_winner(a, pi[0], ps[0], b[0].obj, b[0].prev, b[0].key);
            if (win1) apply_winner(a, pi[1], ps[1], b[1].obj, b[1].prev, b[1].key);
        }
        K = two_pass_on(pi, ps, win0, win1, {b[0].prev, b[1].prev}, {b[0].pstart, b[1].pstart});
        const bool done = K <= 1 || nits >= max_iter;
        // the early request assumed "both bidders win, nobody moves"; otherwise (a scanned row, a lost bid, the
        // end of a chain) request again
        if (!done && (sp[0] != pi[0] || sp[1] != pi[1])) request_two(a, ed, pi[0], ps[0], pi[1], ps[1], tf);
        if (bd_person >= 0) tail_build(a, bd_person, bd, eps, st);
        stamp.light(6);
        if (done) break;
    }
    if (K == 1 && nits < max_iter) tail_chain_mode(a, ed, pi[0], ps[0], K, nits, max_iter, eps, st);
#ifdef MISSLAP_TAIL_STAMP_SOLO
    if (lane == 0)
        for (int k = 1; k <= 6; ++k) a.ctl->dbg[5 + k] += sacc[k];
#endif
    two_hand_back(sU, sStart, pi, ps);
}

// lane-wise values that a round forms under its record gather: the empty statement defines them at this point of the
// program, so the compiler cannot sink the instructions that form them into the instruction-bound part of the round
__device__ __forceinline__ void pin_here(int &a, int &b, int &c, double &d) {
    int lo = __double2loint(d), hi = __double2hiint(d);
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(lo), "+v"(hi));
    d = __hiloint2double(hi, lo);
}

// ---- pair mode: K == 2, handles with lines ---------------------------------------------------------------------------
// Wavefront 0 alone, in the form of the chain round: person A's line in lanes 0..31, person B's in lanes 32..63, ONE line
// load, ONE record gather and ONE evaluation serve both bids; no LDS, no barrier.  Per half the chain's "winner first"
// shortcut: one 32-bit reduction of the values' high words (half_allmax_i32: every lane holds its half's maximum), one
// ballot, popc / ffs per half; the exact 64-bit passes only when a half has a tie on the high word.  Both next lines
// are requested with one load as soon as both winners are known ("both bidders win, nobody moves").
// Both bids use the prices of the previous round: this round's records are stored after both bids are formed, and the
// next gather follows those stores in program order (the wavefront's memory path is in order), so nothing gathered
// ahead has to be patched.  A clean round -- two different objects, both owned: 99.9 % -- needs no RESOLVE: both
// bidders win, each slot passes to the owner its bidder evicts (:409), and both records go out as ONE store by the two
// winning lanes.  Any other round runs RESOLVE (:375-385, strict ">": the earlier list position keeps an object on equal
// bids), ASSIGN (:396-418) and push_all_left on two slots (:137-162) as tail_solo_mode does.  A line that does not
// decide is answered by a full scan of the row, and the line is rebuilt, inside the miss block.  When K falls to 1 the
// wavefront goes on in tail_chain_mode.
// The evaluation is lane-wise (device_common.hpp: cand_eval1_lane, here for both halves in the same instructions): the
// lane that holds its half's winning candidate forms the bid and the hit test against its half's tau and stores
// {bid, its half's bidder, that bidder's row start} at its own column.  No per-half scalar is formed on the clean path:
// wave-uniform are the two owners (read out in front of the request), "both lines decided" (one ballot), the two objects
// of the clean test and the next row starts.
template <class E>
__device__ __forceinline__ void tail_pair_mode(const TailArgs &a, const E &ed, int *sU, int *sStart, int &K,
                                               long long &nits, const long long max_iter, const double eps,
                                               TailStats &st) {
    const int lane = lane_id(), l32 = lane & (kCandLanes - 1);
    const bool upper = lane >= kCandLanes;  // the lane serves slot 1
    const RecSource src{a.rec};
    const bool cls = (l32 >= 1) & (l32 <= kCandMax);
    const double ninf = -__builtin_huge_val();
    int pi[2], ps[2];
#pragma unroll
    for (int X = 0; X < 2; ++X) {
        pi[X] = __builtin_amdgcn_readfirstlane(sU[X]);
        ps[X] = __builtin_amdgcn_readfirstlane(sStart[X]);
    }
    typename E::Slot slot;
    auto request = [&](int p0, int p1) { slot = line_of<E>(a, upper ? p1 : p0, l32); };
    const int rmax = round_limit(nits, max_iter);
    int r = 0;
    if (K == 2) request(pi[0], pi[1]);
#ifdef MISSLAP_TAIL_STAMP_DUO
    // diagnostic build: cycles per segment of a K = 2 round -> Ctl::dbg[6..11]: [6] wait for the lines, [7] record gather,
    // [8] both winners known + next lines requested, [9] rest of the evaluation, [10] full scans of missed persons,
    // [11] resolve / stores / re-request
    unsigned long long sacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sprev = __builtin_amdgcn_s_memtime();
    const CycleStamp stamp{sacc, &sprev, true};
#else
    const NoStamp stamp;
#endif
    while (K == 2) {  // (wave-uniform: the loop ends by `break`)
        stamp(1);
        const PriceRec g = cand_gather1(slot, cls, src);
        // both line evaluations in the lane-wise form of cand_eval1_lane, both halves in the same instructions.  Under the
        // gather: what needs the lines and the bidders alone, for the lane's half
        const bool is_cand = cls & (slot.x >= 0);
        const double cost = slot_cost_or_ninf(slot, is_cand);
        int obj = copy_here(slot.x);  // (the next lines overwrite `slot`)
        double tau[2];
        int len[2];
#pragma unroll
        for (int X = 0; X < 2; ++X) {
            tau[X] = readlane_f64(__hiloint2double(slot.y, slot.x), kCandLanes * X);
            len[X] = __builtin_amdgcn_readlane(slot.x, kCandLanes * X + kCandLanes - 1);
        }
        double tauL = upper ? tau[1] : tau[0];
        int piL = upper ? pi[1] : pi[0], psL = upper ? ps[1] : ps[0];
        pin_here(obj, piL, psL, tauL);  // (formed HERE, where the wavefront waits anyway, not where they are first used)
        stamp(2);
        const double v = cost - g.price;  // vi = cost - p[j]   (:350); -inf where the lane holds no candidate
        const int hw = __double2hiint(v);
        const int k = hw ^ ((hw >> 31) & 0x7fffffff);  // signed order of k == order of the doubles' high words
        const bool top = k == half_allmax_i32(k);
        const unsigned long long eq = __ballot(top);
        const unsigned eq0 = (unsigned)eq, eq1 = (unsigned)(eq >> 32);
        int sl[2];  // winning lane of each half (the half's lane 0: no candidate)
        bool mine;  // the lane holds its half's winning candidate
        if ((int)(__popc(eq0) == 1) & (int)(__popc(eq1) == 1)) {  // wave-uniform, the common case
            sl[0] = __ffs((int)eq0) - 1;
            sl[1] = __ffs((int)eq1) + (kCandLanes - 1);
            mine = top;
        } else {  // a tie on the high word: the exact passes (for both halves, in the same instructions)
            const double vm = half_max_f64(v);
            const double V0 = readlane_f64(vm, kCandLanes - 1), V1 = readlane_f64(vm, kWave - 1);
            const int gm = half_max_i32((is_cand & (v == (upper ? V1 : V0))) ? lane : -1);  // the LAST slot holding it
            const int G0 = __builtin_amdgcn_readlane(gm, kCandLanes - 1), G1 = __builtin_amdgcn_readlane(gm, kWave - 1);
            mine = lane == (upper ? G1 : G0);  // (-1: no candidate, no lane)
            sl[0] = max(G0, 0);
            sl[1] = max(G1, kCandLanes);
        }
        // in front of the request only the two owners are read out: the persons whose lines are requested early
        const int sp0 = __builtin_amdgcn_readlane(g.owner, sl[0]), sp1 = __builtin_amdgcn_readlane(g.owner, sl[1]);
        request(sp0, sp1);  // `slot` is dead from here on
        stamp.light(3);
        const double W = half_allmax_f64(mine ? ninf : v);  // second best of the lane's half, counting multiplicity
        double bid = (cost - W) + eps;                      // bbest = costbest - wi + eps   (:360), in the winners' lanes
        const bool hit = mine & (v > tauL) & (W >= tauL);
        st.bad_hi = max(st.bad_hi, hit ? (unsigned)__double2hiint(bid) : 0u);  // (per lane, see cand_eval1_lane)
        const unsigned long long hm = __builtin_amdgcn_ballot_w64(hit);  // (at most one lane per half)
        // wave-uniform is what control flow needs: the clean test's two objects (the owners are already held) and the next
        // row starts
        int o[2], prev[2] = {sp0, sp1}, pst[2];
#pragma unroll
        for (int X = 0; X < 2; ++X) {
            o[X] = __builtin_amdgcn_readlane(obj, sl[X]);
            pst[X] = __builtin_amdgcn_readlane(g.ostart, sl[X]);
        }
        bool store = mine;  // the lanes that hold a half's result {object, bid}: ASSIGN is one store by them
        stamp.light(4);
        if (__popcll(hm) != 2) {  // wave-uniform (rare behind the maintenance pass): a line did not decide.  The scan and
                                  // the line's rebuild stay inside this block; a scan's result is wave-uniform, so from
                                  // here on lanes 0 and 32 hold the halves' results
            CandBid b[2];
#pragma unroll
            for (int X = 0; X < 2; ++X) {
                b[X].hit = (unsigned)(hm >> (kCandLanes * X)) != 0u;
                b[X].key = bid_to_key(readlane_f64(bid, sl[X]));
                b[X].obj = o[X];
                b[X].prev = prev[X];
                b[X].pstart = pst[X];
                b[X].len = len[X];
            }
#pragma unroll
            for (int X = 0; X < 2; ++X) {
                if (!b[X].hit) {
                    CandBuildArgs bd;
                    tail_scan(a, ed, ps[X], a.row_ptr[pi[X] + 1], eps, b[X], bd, st);
                    if (bd.want) tail_build(a, pi[X], bd, eps, st);
                }
                o[X] = b[X].obj;
                prev[X] = b[X].prev;
                pst[X] = b[X].pstart;
                len[X] = b[X].len;
                sl[X] = kCandLanes * X;
            }
            store = l32 == 0;
            bid = key_to_bid(upper ? b[1].key : b[0].key);
            obj = upper ? b[1].obj : b[0].obj;
        }
        stamp.light(5);
        st.edges += (unsigned long long)(len[0] + len[1]);
        st.bids += 2;
        r += 1;
        if ((int)(o[0] != o[1]) & (int)(prev[0] >= 0) & (int)(prev[1] >= 0)) {  // wave-uniform
            // CLEAN: both bidders win (:375-385 has nothing to resolve); ASSIGN (:396-418) of both as ONE store by the two
            // lanes that hold the results, straight from their registers; each slot passes to the owner its bidder evicts
            // (:409)
            if (store) {
                PriceRec n;
                n.price = bid;
                n.owner = piL;
                n.ostart = psL;
                a.rec[(unsigned)obj] = n;  // (an object: >= 0, no sign extension)
            }
#pragma unroll
            for (int X = 0; X < 2; ++X) {
                pi[X] = prev[X];
                ps[X] = pst[X];
            }
        } else {
            // RESOLVE (:375-385): strict ">" -- the earlier list position keeps an object on equal bids.  The keys are read
            // out of the lanes here, where they are needed
            bool win0 = true, win1 = true;
            if (o[0] == o[1])
                two_resolve(bid_to_key(readlane_f64(bid, sl[0])), bid_to_key(readlane_f64(bid, sl[1])), win0, win1);
            // ASSIGN (:396-418) stays lane-wise: the winners' lanes store from their own registers
            if (store & (upper ? win1 : win0)) {
                PriceRec n;
                n.price = bid;
                n.owner = piL;
                n.ostart = psL;
                a.rec[(unsigned)obj] = n;
            }
            K = two_pass_on(pi, ps, win0, win1, prev, pst);
        }
        const bool done = K <= 1 || r >= rmax;
        // the early request assumed "both bidders win, nobody moves"; otherwise (a scanned row that decided differently
        // from its line, a lost bid, the end of a chain) request again
        if (!done && (sp0 != pi[0] || sp1 != pi[1])) request(pi[0], pi[1]);
        stamp.light(6);
        if (done) break;
    }
    nits += r;
#ifdef MISSLAP_TAIL_STAMP_DUO
    if (lane == 0)
        for (int k = 1; k <= 6; ++k) a.ctl->dbg[5 + k] += sacc[k];
#endif
    if (K == 1 && nits < max_iter) tail_chain_mode(a, ed, pi[0], ps[0], K, nits, max_iter, eps, st);
    two_hand_back(sU, sStart, pi, ps);
}

// ---- team mode: 3 <= K <= 16 -----------------------------------------------------------------------------------
// Wavefront w serves list slots 2w and 2w + 1 (the two halves of its lines).  ONE barrier per round: the bids AND the
// bidders go to LDS (double-buffered by round parity), and behind the barrier EVERY wavefront finishes the round for
// the whole list redundantly on lanes = slots, so nobody waits for a resolver and no second barrier publishes a
// result.  Every serving wavefront stores the records of ALL winners itself (identical values from every wavefront):
// its own next gathers then follow its own stores in program order, which is the only ordering a wavefront's
// in-order memory path gives for free -- and the barrier guarantees that every wavefront has finished the gathers of
// the round before anybody stores.
// Almost every round is "clean": no object is bid on twice and no chain ends (no bidder wins an unowned object).
// Then every bidder wins, every slot passes to the owner its bidder evicts (:409), the list keeps its length and
// order, and a wavefront already knows its own next persons -- their lines were requested when the winning
// candidates were known.  The clean test is one LDS compare-and-swap per slot (a private 64-entry table per
// wavefront: an insert that meets its own object = a contested object) and one ballot; only an unclean round runs
// RESOLVE (:375-385) / push_all_left (:137-162) in full.
constexpr int kTeamMax = 16;
constexpr int kTeamTab = 64;  // entries of a wavefront's private duplicate-detection table (<= 16 inserts)
__device__ __forceinline__ void tail_barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <class E>
__device__ __forceinline__ void tail_team_mode(const TailArgs &a, const E &ed, int *sU, int *sStart, int &K,
                                               long long &nits, const long long max_iter, const double eps,
                                               TailStats &st) {
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    static_assert(kTeamMax <= 2 * (kTailMax / kWave) && kTeamMax <= kWave, "two list slots per wavefront");
    __shared__ unsigned long long tKey[2][kTeamMax];
    __shared__ int tObj[2][kTeamMax], tPrev[2][kTeamMax], tPst[2][kTeamMax], tU[2][kTeamMax], tS[2][kTeamMax];
    __shared__ int wTab[kTailMax / kWave][kTeamTab];
    const int n0 = 2 * wave;  // my slots: n0, n0 + 1
    int pi[2], ps[2];
#pragma unroll
    for (int X = 0; X < 2; ++X) {
        pi[X] = n0 + X < K ? __builtin_amdgcn_readfirstlane(sU[min(n0 + X, kTailMax - 1)]) : -1;
        ps[X] = n0 + X < K ? __builtin_amdgcn_readfirstlane(sStart[min(n0 + X, kTailMax - 1)]) : 0;
    }
    wTab[wave][lane & (kTeamTab - 1)] = -1;
    TwoFetch<E> tf;
    tf.slot = cand_no_line<typename E::Slot>();
    if (n0 < K) request_two(a, ed, pi[0], ps[0], pi[1], ps[1], tf);
    __syncthreads();  // (sU / sStart have been read by everybody)
#ifdef MISSLAP_TAIL_STAMP_TEAM
    // diagnostic build: cycles of wavefront 0 per segment of a team round -> Ctl::dbg[6..9]: [6] bids of my slots,
    // [7] barrier, [8] clean test / resolve / assign, [9] re-request, line rebuild
    unsigned long long sacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sprev = __builtin_amdgcn_s_memtime();
    const CycleStamp stamp{sacc, &sprev, wave == 0};
#else
    const NoStamp stamp;
#endif
    int par = 0;
    for (;;) {
        int sp[2] = {-2, -2};  // persons whose lines were requested early (-2: nothing requested)
        CandBuildArgs bd;
        int bd_person = -1;
        stamp.light(0);
        if (n0 < K) {  // wave-uniform: BID for my slots (slots < K are always occupied: the list is compact)
            CandBid b[2];
            bid_two(a, ed, pi, ps, tf, eps, b, bd, bd_person, st, [&](const CandBid(&w)[2]) {
                sp[0] = pi[0] >= 0 ? w[0].prev : -1;
                sp[1] = pi[1] >= 0 ? w[1].prev : -1;
                request_two(a, ed, sp[0], 0, sp[1], 0, tf);  // the owners my bidders evict if they win
            });
            if (lane == 0) {
#pragma unroll
                for (int X = 0; X < 2; ++X)
                    if (pi[X] >= 0) {
                        tKey[par][n0 + X] = b[X].key;
                        tObj[par][n0 + X] = b[X].obj;
                        tPrev[par][n0 + X] = b[X].prev;
                        tPst[par][n0 + X] = b[X].pstart;
                        tU[par][n0 + X] = pi[X];
                        tS[par][n0 + X] = ps[X];
                    }
            }
        }
        stamp.light(1);
        tail_barrier_lds();  // the bids are in LDS and every gather of the round is done; requests stay in flight
        stamp.light(2);
        {
            const bool act = lane < K;
            const int ls = min(lane, kTeamMax - 1);
            const unsigned long long lkey = act ? tKey[par][ls] : 0ull;
            const int lobj = act ? tObj[par][ls] : (-2 - lane);
            const int lprev = act ? tPrev[par][ls] : 0, lpst = act ? tPst[par][ls] : 0;
            int u = act ? tU[par][ls] : -1;  // the list: lane l holds slot l
            int sx = act ? tS[par][ls] : 0;
            // clean round?  (a) no object bid on twice: one compare-and-swap per slot into my private table
            int hs = 0;
            bool dup = false;
            if (act) {
                hs = (int)(((unsigned)lobj * 2654435761u) >> 26) & (kTeamTab - 1);
                for (;;) {
                    const int old = atomicCAS(&wTab[wave][hs], -1, lobj);
                    if (old == -1) break;
                    if (old == lobj) {
                        dup = true;
                        break;
                    }
                    hs = (hs + 1) & (kTeamTab - 1);
                }
            }
            const bool contested = __any(dup);
            if (act && !dup) wTab[wave][hs] = -1;  // (LDS operations of a wavefront complete in order)
            // (b) no chain ends
            const bool ends = __any(act && lprev == -1);
#ifdef MISSLAP_TAIL_STAMP_TEAM
            if (threadIdx.x == 0) sacc[5] += (!contested && !ends), sacc[6] += contested, sacc[7] += 1;
#endif
            if (!contested && !ends) {
                // every bidder wins (:375-385 has nothing to resolve); ASSIGN (:396-418); the list keeps its shape
                if (act && n0 < K) apply_winner(a, u, sx, lobj, lprev, lkey);
#pragma unroll
                for (int X = 0; X < 2; ++X) {
                    const int w = __builtin_amdgcn_readlane(lprev, min(n0 + X, kWave - 1));
                    const int ws = __builtin_amdgcn_readlane(lpst, min(n0 + X, kWave - 1));
                    pi[X] = n0 + X < K ? w : -1;
                    ps[X] = n0 + X < K ? ws : 0;
                }
            } else {
                // RESOLVE / ASSIGN / push_all_left in full, on lanes = slots
                const bool won = act && !lanes_lose(lobj, lkey, K, lane);
                if (won && n0 < K) apply_winner(a, u, sx, lobj, lprev, lkey);  // :396-418 (serving wavefronts only)
                u = won ? lprev : u;  // the evicted owner inherits the slot (:409) / hole (:412) / a loser stays
                sx = won ? lpst : sx;
                K = lanes_push_left(u, sx, act, K, lane);
#pragma unroll
                for (int X = 0; X < 2; ++X) {
                    pi[X] = n0 + X < K ? __builtin_amdgcn_readlane(u, min(n0 + X, kWave - 1)) : -1;
                    ps[X] = n0 + X < K ? __builtin_amdgcn_readlane(sx, min(n0 + X, kWave - 1)) : 0;
                }
            }
        }
        stamp.light(3);
        par ^= 1;
        nits += 1;
        const bool done = K <= 2 || nits >= max_iter;
        // my slots' new occupants are usually exactly the persons whose lines were requested early; otherwise (a
        // scanned row, a lost bid, a moved person) request now
        if (!done && n0 < K && (sp[0] != pi[0] || sp[1] != pi[1]))
            request_two(a, ed, pi[0], ps[0], pi[1], ps[1], tf);
        if (bd_person >= 0) tail_build(a, bd_person, bd, eps, st);
        stamp.light(4);
        if (done) break;
    }
#ifdef MISSLAP_TAIL_STAMP_TEAM
    if (threadIdx.x == 0)
        for (int k = 1; k <= 6; ++k) a.ctl->dbg[5 + k] += sacc[k];
#endif
    // hand the list back: every wavefront writes its own slots
    if (lane < 2 && n0 + lane < kTeamMax) {
        sU[n0 + lane] = lane == 0 ? pi[0] : pi[1];
        sStart[n0 + lane] = lane == 0 ? ps[0] : ps[1];
    }
    __syncthreads();
}

// ---- the team rounds of handles with lines: few instructions, one barrier, the next gather issued ahead ----------------
// A wavefront of the tail issues one instruction every ~8 cycles whatever the instruction is (tools/micro/
// exec_mask_bench.hip: dependent VALU 8.2 cycles, independent 6.1; profiles/r06_tail_overheads.txt), so a round is as long
// as the instructions on its wavefront plus the memory waits it cannot hide.  What a team round does BESIDES the
// evaluation of its line is therefore written to be few instructions:
//   * a slot publishes TWO 16-byte LDS entries ahead of the barrier: the price record its winning bid would write
//     {bid, bidder, bidder's row start} and {object, its owner, the owner's row start};
//   * the clean test -- no object bid on twice, no chain ends (an unowned object won): 99.9 % of the rounds -- moves IN
//     FRONT of the barrier: each bidder swaps the round's number into a table slot keyed by its object's hash (one
//     ds_wrxchg per wavefront; meeting the round's own number = two bids on one hash) and writes the round's number into
//     the dirty word of the round's parity if that, or the end of a chain, is seen.  Behind the barrier the test is ONE
//     broadcast LDS read.  Round numbers only grow, so neither the table nor the dirty words are ever reset; a false
//     positive (two objects, one hash: < 1 % of the rounds) only sends the round through the exact RESOLVE / ASSIGN /
//     push_all_left (auction_.pyx:375-385 strict ">", :396-418, :137-162), which is the code every round ran before;
//   * in a clean round every bidder wins and every slot passes to the owner its bidder evicts (:409): a wavefront's next
//     bidder is in its own registers, and ALL winners' records are one 16-byte store on lanes = slots (every serving
//     wavefront stores them all itself: its later gathers follow them in program order);
//   * the record gather of the NEXT bid is issued AHEAD of the barrier, as soon as the next bidder's line has landed, and
//     made exact behind it: a candidate whose object was bid on in this round takes the PUBLISHED record (whether the
//     gather saw the old or the new one does not matter); every other record cannot have changed (:394-427 writes only
//     the objects bid on), and the next round's stores lie behind ITS barrier, which no wavefront reaches before its
//     gather has landed.  "Bid on in this round" is read off the same hash table (own object: patched from registers;
//     any other hit -- rare -- walks the published slots);
//   * rounds are counted in 32 bits inside a mode (a launch is bounded by TailArgs::round_budget / 2^31 rounds) and the
//     statistics that can be derived (line hits = bids - misses) are not counted;
//   * wavefronts whose slot lies beyond K (K never grows) END after one more barrier: the barrier is then between the
//     serving wavefronts only.
constexpr int kPipeTab = 4096;  // (K = 16: 3 % false positives of the clean test, K = 6: 0.4 %)
__device__ __forceinline__ int pipe_hash(int obj) { return (int)(((unsigned)obj * 2654435761u) >> 20); }
static_assert((1 << 12) == kPipeTab, "pipe_hash keeps the top 12 bits");
struct __attribute__((aligned(16))) PipeSlot {
    PriceRec rec;  // what the slot's winning bid writes: {bid, bidder, bidder's row start}
    int4 aux;      // {object bid on, its owner, the owner's row start, -}
};
struct __attribute__((aligned(16))) PipeLds {
    PipeSlot slot[2][kTeamMax];  // by round parity
    int dirty[2];                // number of the last round (of this parity) that needs the exact RESOLVE
    int pad[2];
    int tab[kPipeTab];           // hash of an object -> number of the last round in which it was bid on
};

// (a line's registers are "used" here so that the compiler's wait for the line load sits AT this point: what is issued
// behind it -- the winners' stores -- is then not in front of any later wait for the line)
__device__ __forceinline__ void touch_slot(const int2 &s) { asm volatile("" ::"v"(s.x), "v"(s.y)); }
__device__ __forceinline__ void touch_slot(const Slot64 &s) { asm volatile("" ::"v"(s.x), "v"(s.y), "v"(s.c)); }

// returns true when this wavefront has LEFT (its slot lies beyond K): the caller flushes its statistics and ends
template <class E>
__device__ __forceinline__ bool tail_team1_pipe(const TailArgs &a, const E &ed, int *sU, int *sStart, int &K,
                                                long long &nits, const long long max_iter, const double eps,
                                                TailStats &st) {
    const int lane = lane_id(), l32 = lane & (kCandLanes - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    __shared__ PipeLds L;
    const RecSource src{a.rec};
    const bool cls = (lane >= 1) & (lane <= kCandMax);
    const int n0 = wave;  // my slot
    int pi = n0 < K ? __builtin_amdgcn_readfirstlane(sU[min(n0, kTeamMax - 1)]) : -1;  // (the list has kTeamMax slots)
    int ps = n0 < K ? __builtin_amdgcn_readfirstlane(sStart[min(n0, kTeamMax - 1)]) : 0;
    for (int h = threadIdx.x; h < kPipeTab; h += blockDim.x) L.tab[h] = -1;  // (round numbers are >= 0)
    if (threadIdx.x < 2) L.dirty[threadIdx.x] = -1;
    typename E::Slot slot = cand_no_line<typename E::Slot>();
    auto request = [&](int person) { slot = line_of<E>(a, person, l32); };
    if (n0 < K) request(pi);
    __syncthreads();  // (sU / sStart have been read by everybody, the tables are set)
#ifdef MISSLAP_TAIL_STAMP_TEAM
    // diagnostic build: cycles of wavefront 0 per segment of a team round -> Ctl::dbg[6..11]: [6] wait for the line + record
    // gather, [7] evaluation of my slot up to the bid, [8] publish, [9] barrier, [10] LDS reads landed, [11] dirty word /
    // stores / re-request / loop
    unsigned long long sacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sprev = __builtin_amdgcn_s_memtime();
    const CycleStamp stamp{sacc, &sprev, wave == 0};
#else
    const NoStamp stamp;
#endif
    const int rmax = round_limit(nits, max_iter);
    int r = 0;  // rounds done here = the round's number
    int par = 0;
    const int ls = min(lane, kTeamMax - 1);
    PriceRec grec = PriceRec{0.0, -1, 0};
    bool have_g = false;  // the records of my slot's line have been requested (behind the previous round's stores)
    for (;;) {
        if (n0 >= K) {  // wave-uniform: my slot fell away (slots < K are always occupied: the list is compact)
            if (lane == 0) {
                sU[n0] = -1;  // (I end behind this barrier; the serving wavefronts hand their slots back)
                sStart[n0] = 0;
            }
            tail_barrier_lds();
            nits += r;
            return true;
        }
        int sp = -2;  // the person whose line was requested early (-2: nothing requested)
        LaneBid w = {};
        stamp.light(0);
        // BID for my slot (auction_.pyx:339-365).  The gather follows the previous round's stores in program order.
        if (!have_g) grec = cand_gather1(slot, cls, src);
#ifdef MISSLAP_TAIL_STAMP_TEAM
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp.light(1);
#endif
        cand_eval1_lane(slot, grec, cls, eps, w, st.bad_hi, [&](int prev) {
            sp = prev;
            request(sp);  // the owner my bidder evicts if it wins
        });
        // The lane that holds the winning candidate publishes the bid and exchanges the clean test's tag, from the
        // registers it already holds: {bid, bidder, bidder's row start} and {object, its owner, the owner's row start}
        bool publish = w.mine;
        double bid = w.bid;
        int obj = w.obj, own = grec.owner, ost = grec.ostart, len = w.len;
        int nprev = w.prev, npst = w.pstart;  // my slot's next occupant if my bidder wins: the owner it evicts
        if (!w.hit) {  // wave-uniform (rare behind the maintenance pass: the scan and the line's rebuild stay inside this
                       // block); the scan's result is wave-uniform and lane 0 publishes it
            CandBid b;
            CandBuildArgs bd;
            tail_scan(a, ed, ps, a.row_ptr[pi + 1 + lane_zero()], eps, b, bd, st);
            if (bd.want) tail_build(a, pi, bd, eps, st);
            publish = lane == 0;
            bid = key_to_bid(b.key);
            obj = b.obj;
            own = nprev = b.prev;
            ost = npst = b.pstart;
            len = b.len;
        }
        st.edges += (unsigned long long)len;
        st.bids += 1;
        stamp.light(2);
        if (publish) {
            const int old = atomicExch(&L.tab[pipe_hash(obj)], r);
            PriceRec mine;
            mine.price = bid;
            mine.owner = pi;
            mine.ostart = ps;
            L.slot[par][n0].rec = mine;
            L.slot[par][n0].aux = make_int4(obj, own, ost, 0);
            if (old == r || own < 0) L.dirty[par] = r;
        }
        stamp.light(3);
        tail_barrier_lds();  // the bids are in LDS and every gather of the round has landed
        stamp.light(4);
        {
            const int dflag = L.dirty[par];
            const PriceRec lrec = L.slot[par][ls].rec;  // lanes = slots
            const int lobj = L.slot[par][ls].aux.x;
#ifdef MISSLAP_TAIL_STAMP_TEAM
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            stamp.light(5);
#endif
            if (__builtin_amdgcn_readfirstlane(dflag) != r) {
                // CLEAN: every bidder wins (:375-385 has nothing to resolve); ASSIGN (:396-418) of every slot on lanes =
                // slots; the list keeps its shape and my slot passes to the owner my bidder evicts (:409), whose line was
                // requested when the winner was known: it has been in flight behind the rest of the evaluation, the
                // publish, the barrier and these reads
                // (the next gather is issued right here, behind the stores and inside the block that has waited for the line:
                // at the loop's back edge the compiler would put a wait for EVERYTHING in front of it, the stores included)
                have_g = sp == nprev;  // (wave-uniform; false only behind a scanned row that decided differently from its line)
                if (have_g) {
                    touch_slot(slot);
                    if (lane < K) a.rec[lobj] = lrec;
                    grec = cand_gather1(slot, cls, src);
                } else {
                    if (lane < K) a.rec[lobj] = lrec;
                }
                pi = nprev;
                ps = npst;
            } else {
                // RESOLVE / ASSIGN / push_all_left in full, on lanes = slots
                have_g = false;
                const bool act = lane < K;
                const int4 laux = L.slot[par][ls].aux;
                const unsigned long long lkey = act ? bid_to_key(lrec.price) : 0ull;
                const int lo = act ? laux.x : (-2 - lane);
                const int lprev = act ? laux.y : 0, lpst = act ? laux.z : 0;
                int u = act ? lrec.owner : -1;  // the list: lane l holds slot l
                int sx = act ? lrec.ostart : 0;
                const bool won = act && !lanes_lose(lo, lkey, K, lane);
                if (won) apply_winner(a, u, sx, lo, lprev, lkey);  // :396-418
                u = won ? lprev : u;  // the evicted owner inherits the slot (:409) / hole (:412) / a loser stays
                sx = won ? lpst : sx;
                K = lanes_push_left(u, sx, act, K, lane);
                pi = n0 < K ? __builtin_amdgcn_readlane(u, min(n0, kWave - 1)) : -1;
                ps = n0 < K ? __builtin_amdgcn_readlane(sx, min(n0, kWave - 1)) : 0;
            }
        }
        par ^= 1;
        r += 1;
        const bool done = K <= 2 || r >= rmax;
        // my slot's new occupant is usually exactly the person whose line was requested early; otherwise (a scanned
        // row, a lost bid, a moved person) request now
        if (!done && n0 < K && sp != pi) request(pi);
        stamp.light(6);
        if (done) break;
    }
    nits += r;
#ifdef MISSLAP_TAIL_STAMP_TEAM
    if (threadIdx.x == 0)
        for (int k = 1; k <= 6; ++k) a.ctl->dbg[5 + k] += sacc[k];
#endif
    // hand the list back: every wavefront that is still here writes its own slot
    if (lane == 0 && n0 < kTeamMax) {
        sU[n0] = pi;
        sStart[n0] = ps;
    }
    __syncthreads();
    return false;
}

// ---- the clean test of a block round (17 <= K <= 192 bidders at the default threshold) -------------------------------
// As in the team rounds, almost every block round is clean -- no object bid on twice, no unowned object won (C3: 93 % of
// the block rounds, profiles/tail_block_clean.txt) -- and then every bidder wins, every slot passes to the owner its bidder
// evicts (:409) and the list keeps its length and order: nothing is left to RESOLVE (:375-385) or to push left (:137-162).
// The test runs IN FRONT of the barriers, by the lanes that publish a slot.  A table of one-probe tags (the team rounds'
// kPipeTab) cannot serve 192 bidders: 192 objects fall on 192 different tags of a table of T entries with probability
// exp(-192 * 191 / 2T), i.e. 67 % false positives at T = 16384 (64 KB), 11 % at K = 64.  The table below is therefore EXACT:
// an entry is {round tag, object} as one 64-bit key, inserted with one LDS atomic maximum at the object's hash.  Tags
// only grow, so an entry of an earlier round is smaller than every key of this one: the maximum replaces it and returns it
// -- the slot was free, one LDS operation, the common case.  Meeting the own key = the object has been bid on in this
// round.  Meeting another key of this round (two objects, one hash: 9 % of the inserts at K = 192, 0.8 % at K = 17): the
// slot keeps the larger of the two keys and the lane carries the smaller one to the next slot (an ordered open-addressing
// table: the slots between an object's hash and its key hold larger keys of this round, and entries only grow within a
// round, so a second bid on the object walks the same slots and meets the key -- or a lane that carries it meets the
// second bid's).  No round resets anything.  A walk that has not ended after kCleanProbes slots reports "bid on twice",
// which only sends the round through the exact path.
// The table lives in hKey, the key array of the exact path's own hash table (64 < K): both are empty at zero, the exact
// path empties the array before it inserts and leaves it empty.  A table of its own (32 KB more) takes the workgroup's
// LDS beyond 64 KB, where an address no longer fits the LDS instructions' offset field and every array costs an address
// register: the 1024-thread kernels then spill (16 .. 60 bytes of scratch per lane).
constexpr int kCleanTab = kHashSize;
constexpr int kCleanProbes = 8;
static_assert(2 * kCleanTab == kPipeTab, "clean_hash: pipe_hash's top 11 bits");
__device__ __forceinline__ int clean_hash(int obj) { return pipe_hash(obj) >> 1; }
// The thread's slot index, formed HERE: the LDS addresses of a block of slot-indexed accesses are then computed inside the
// block, from one register and the arrays' offsets.  Left to itself the compiler forms one address register per array ahead of
// the round loop and keeps them all for the whole kernel, which the 1024-thread kernels (128 VGPRs) pay with spills.
__device__ __forceinline__ int slot_index_here(int t) {
    asm volatile("" : "+v"(t));
    return t;
}
// LDS reads issued together are waited for HERE, together (the two values stand for their group: the LDS returns in order),
// so that a branch behind them costs no second LDS latency
__device__ __forceinline__ void lds_landed_here(int &a, int &b) { asm volatile("" : "+v"(a), "+v"(b)); }
// true: `obj` has been bid on before in the round `tag` (or the walk was cut short)
__device__ __forceinline__ bool clean_insert(unsigned long long *tab, unsigned tag, int obj) {
    const unsigned long long first = (unsigned long long)tag << 32;
    unsigned long long cur = first | (unsigned long long)(unsigned)obj;
    int h = clean_hash(obj);
    for (int probe = 0; probe < kCleanProbes; ++probe) {
        const unsigned long long old = atomicMax(&tab[h], cur);
        if (old < first) return false;                              // an entry of an earlier round: the slot was free
        if (old == cur || (unsigned)(old >> 32) != tag) return true;  // (a larger tag: the 32-bit round count has wrapped)
        cur = min(old, cur);  // two objects, one hash: the smaller key moves on
        h = (h + 1) & (kCleanTab - 1);
    }
    return true;
}

// ---- what every tail kernel does at its start and at its end -------------------------------------------------------------
// what a kernel carries from tail_begin to tail_end
struct TailRun {
    int K, K0;
    long long nits, nits0, max_iter;
    double eps;
    TailStats st;
    // per-mode accounting (always on: two s_memrealtime reads per mode entry -- block mode: per ROUND; bracketing a whole
    // run of block rounds instead was measured 1.3 ms per C3 solve slower, profiles/tail_block_lane.txt --, 100 MHz
    // ticks), Ctl::dbg:
    //   [0..2] rounds in chain + pair + solo / team / block mode, [3..5] ticks
    unsigned long long md[6];
    __device__ __forceinline__ void mode_begin(int m) {
        md[3 + m] -= __builtin_amdgcn_s_memrealtime();
        md[m] -= (unsigned long long)nits;
    }
    __device__ __forceinline__ void mode_end(int m) {
        md[3 + m] += __builtin_amdgcn_s_memrealtime();
        md[m] += (unsigned long long)nits;
    }
};

// a wavefront's statistics, once, when it leaves the kernel (whole wavefronts call)
__device__ __forceinline__ void tail_flush_stats(Ctl *ctl, TailStats &st) {
    const bool bad_bid = __any(bad_hi_is_error(st.bad_hi));  // (the lane-wise rounds keep the maximum per lane)
    if ((threadIdx.x & 63) == 0) {
        if (st.bids) {
            const unsigned long long hits = (unsigned long long)(st.bids - st.misses), hit_edges = st.edges - st.miss_edges;
            atomicAdd(&ctl->edges, st.edges);
            atomicAdd(&ctl->tail_edges, st.edges);
            atomicAdd(&ctl->bids, (unsigned long long)st.bids);
            if (hits) {
                atomicAdd(&ctl->cand_hits, hits);
                atomicAdd(&ctl->cand_edges, hit_edges);
            }
            atomicAdd(&ctl->dbg[12], (unsigned long long)st.bids);  // the tail's own totals: bids, line hits, line builds
            atomicAdd(&ctl->dbg[13], hits);
            atomicAdd(&ctl->dbg[14], st.builds);
            atomicAdd(&ctl->dbg[15], hit_edges);
        }
        if (bad_bid) st.err |= kErrNegativeBid;
        if (st.err) atomicOr(&ctl->err, st.err);
    }
}

// The start: K / nits, the launch's last round (`budget` > 0: so many rounds from here; 0: no limit), the entry tests
// -- false: these rounds are not this kernel's, return at once; inside a batch every kernel is launched whatever K is,
// and under a budget a kernel that ran out of rounds leaves K to the NEXT launch's kernel of the right role --, the list
// into sU / sStart[0, slots), the statistics zeroed.  The caller sets its own LDS and closes with the barrier.
__device__ __forceinline__ bool tail_begin(const TailArgs &a, int budget, int k_lo, int k_hi, int *sU, int *sStart,
                                           int slots, int threads, TailRun &r) {
    const Ctl *ctl = a.ctl;
    r.K = ctl->K;
    r.nits = ctl->nits;
    r.max_iter = budget > 0 ? min(ctl->max_iter, r.nits + (long long)budget) : ctl->max_iter;
    if (r.K == 0 || r.K > a.thr || r.nits >= r.max_iter) return false;  // uniform
    if (r.K < k_lo || r.K > k_hi) return false;                          // another kernel's rounds
    r.K0 = r.K;
    r.nits0 = r.nits;
    for (int n = threadIdx.x; n < slots; n += threads) {
        sU[n] = (n < r.K) ? a.U[n] : -1;
        sStart[n] = (n < r.K) ? a.row_ptr[sU[n]] : 0;
    }
    r.eps = (double)a.eps;
    r.st = TailStats{};  // (all zero)
    for (int k = 0; k < 6; ++k) r.md[k] = 0ull;
    return true;
}

// The end (every thread that is still here): the mode counters, the list back to U[0, K0), the statistics, K / nits
__device__ __forceinline__ void tail_end(const TailArgs &a, const int *sU, int threads, TailRun &r) {
    Ctl *ctl = a.ctl;
    const int t = threadIdx.x;
    if (t == 0)
        for (int k = 0; k < 6; ++k) ctl->dbg[k] += r.md[k];
    for (int n = t; n < r.K0; n += threads) a.U[n] = sU[n];
    tail_flush_stats(ctl, r.st);
    if (t == 0) {
        ctl->K = r.K;
        ctl->nits = r.nits;
        ctl->tail_rounds += r.nits - r.nits0;
    }
}

// ---- block mode: K > kTeamMax ------------------------------------------------------------------------------------------
// MISSLAP_TAIL_BLOCK_EARLY_SWEEPS is the build switch of the early-sweep A/B, like the MISSLAP_TAIL_STAMP_* ones
// (tools/build_ab.sh es2 "-DMISSLAP_TAIL_BLOCK_EARLY_SWEEPS=2"); above 1 the 12 B/edge k_batched_ptr kernel spills.
#ifndef MISSLAP_TAIL_BLOCK_EARLY_SWEEPS
#define MISSLAP_TAIL_BLOCK_EARLY_SWEEPS 1
#endif
constexpr int kEarlySweeps = MISSLAP_TAIL_BLOCK_EARLY_SWEEPS;  // 0, 1, 2 and all 6 were measured (profiles/tail_block_clean.txt)
constexpr int kEarlyN = kEarlySweeps > 0 ? kEarlySweeps : 1;

// Block rounds until K <= kTeamMax (the next mode takes over), K == 0 or max_iter, on the list sU / sStart[kTailMax].
// kThreads = 1024: SIXTEEN wavefronts -- half the sweeps per wavefront in pass A, which is where a block round spends its
// time; 512: eight, with three sweeps in flight together.  `early_sweeps` (a constant at both call sites): for how many
// sweeps of a round the next lines are requested early; k_tail_block: kEarlySweeps, k_tail_nolines: 0.
// The mode's LDS is declared here, as in the team modes: the two kernels that run block rounds carry it and nobody else
// (a struct like those kernels: the round below stands as it stood in k_tail::run).
template <class E, int kThreads>
struct tail_block_mode {
    static __device__ __forceinline__ void run(const TailArgs &a, const E &ed, int *sU, int *sStart, TailRun &r,
                                               const int early_sweeps) {
        __shared__ unsigned long long sKey[kTailMax];  // per list slot: the bid's key, its object, the object's owner and
        __shared__ int sObj[kTailMax];                 // that owner's row start
        __shared__ int sPrev[kTailMax];
        __shared__ int sPst[kTailMax];
        __shared__ int sList[kTailMax];  // the slots queued for the scan pass; the exact paths' list of holes
        __shared__ int hObj[kHashSize];  // the exact paths' hash table (64 < K), keyed by object
        __shared__ unsigned long long hKey[kHashSize];
        __shared__ int hPos[kHashSize];
        __shared__ int sCnt[3][kThreads / kWave];
        __shared__ unsigned sHit[kTailMax];  // tag of the last block round in which pass A published the slot (a line hit)
        __shared__ unsigned sDirty;  // tag of the last block round that needs the exact RESOLVE / ASSIGN / push_all_left
        __shared__ int sK, sMissCnt;
        unsigned long long *const cTab = hKey;  // the clean table (clean_insert)
        const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
        constexpr int nwaves = kThreads / kWave;
        int &K = r.K;
        long long &nits = r.nits;
        const long long max_iter = r.max_iter;
        const double eps = r.eps;
        TailStats &st = r.st;
        // emptied once per launch: no round resets anything it leaves empty
        for (int n = t; n < kTailMax; n += kThreads) sHit[n] = 0u;  // (round tags are >= 1)
        for (int h = t; h < kHashSize; h += kThreads) {
            hObj[h] = -1;
            hKey[h] = 0ull;
            hPos[h] = kPosNone;
        }
        if (t == 0) sDirty = 0u, sMissCnt = 0;  // (round tags are >= 1; hKey = the clean table is empty at zero)
        __syncthreads();
#ifdef MISSLAP_TAIL_STAMP_BLOCK
        unsigned long long bacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
        // the round's tag in cTab / sDirty, and -- sixteen wavefronts, handles with lines -- per covered sweep the line of
        // the person who takes the sweep's slot of the lane's half if its bidder wins (`enp`; -2: none requested)
        const bool early = early_sweeps > 0;
        unsigned rtag = 0u;
        unsigned long long nclean = 0ull;  // clean block rounds of this launch -> Ctl::dbg[6] (tail_stats[10])
        typename E::Slot el[kEarlyN];
        int enp[kEarlyN];
#pragma unroll
        for (int q = 0; q < kEarlyN; ++q) {
            el[q] = cand_no_line<typename E::Slot>();
            enp[q] = -2;
        }
        for (;;) {
            if (K <= kTeamMax) break;  // the next mode takes over
            // ---- BID in two passes.  Pass A: the lines, two list slots per wavefront (one per 32-lane
            // half, one gather serves both); a hit goes straight to LDS, a miss is queued.  Pass B: the queued persons,
            // one wavefront each, by a full scan of their rows (+ line rebuild).  Between the passes the thread that holds a
            // published slot enters its object into the clean table (a scanned slot's: its scanner) and raises sDirty for a
            // second bid on it or an unowned object (clean_insert).
            // Behind the two passes ONE broadcast LDS read decides: a clean round is finished by the threads = slots
            // (ASSIGN of every bidder, the slot passes to the evicted owner; K and the order stay), every other round by
            // the exact RESOLVE / ASSIGN / push_all_left below.
            // In a clean round slot n's next bidder is the owner in the publishing lane's gathered record, and slot n
            // stays with its wavefront: the first sweep's next lines are requested when the winners are known (early)
            // and are in flight across the LDS-only barriers of both passes, the finish and the closing barrier.  The next
            // round takes such a line only where it belongs to the person its slot then holds -- whatever the round turned
            // out to be; that person did not bid in this round (it owned an object), so no scan pass rebuilt its line.
            r.mode_begin(2);
            rtag += 1u;
#ifdef MISSLAP_TAIL_STAMP_BLOCK
            // diagnostic build: cycles of wavefront 0 per segment of a block round -> Ctl::dbg[6..11]: [6] lines landed
            // (the first sweep's: a requested line only has to finish landing), [7] records landed, [8] evaluated +
            // barrier, [9] clean test + scan pass + barrier, [10] a clean round: the dirty word and the winners' record
            // stores; any other: resolve / assign / compaction, [11] closing barrier
            unsigned long long sprev_b = __builtin_amdgcn_s_memtime();
            const CycleStamp bstamp{bacc, &sprev_b, wave == 0};
#else
            const NoStamp bstamp;
#endif
            {
                const RecSource src{a.rec};
                // kBlockDepth sweeps of 2 * nwaves slots are in flight together: all their lines are requested first,
                // then all record gathers are issued (each as its line lands), then they are evaluated one after the
                // other -- the two memory latencies are paid once per group of sweeps, not once per sweep
                // (sixteen wavefronts -- four per SIMD -- hide the two latencies by themselves: measured per block round
                // 3.51 us with one sweep in flight, 3.69 with two, 3.96 with three, 4.06 with four)
                constexpr int kBlockDepth = kThreads > kTailMax ? 1 : 3;
                const int wv = __builtin_amdgcn_readfirstlane(wave);  // (a scalar: the tests on a wavefront's slots are branches)
                for (int base = 0; base < K; base += kBlockDepth * 2 * nwaves) {
                    typename E::Slot sl[kBlockDepth];
                    PriceRec rr[kBlockDepth];
#pragma unroll
                    for (int c = 0; c < kBlockDepth; ++c) {
                        const int nme = base + c * 2 * nwaves + 2 * wv + (lane >> 5);
                        const int pme = nme < K ? sU[min(nme, kTailMax - 1)] : -1;
                        sl[c] = cand_no_line<typename E::Slot>();
                        if (E::kCand && a.cand != nullptr) {
                            if (early && c == 0 && base < early_sweeps * 2 * nwaves) {  // (wave-uniform) the line requested in the round before
                                int ep = -2;
#pragma unroll
                                for (int q = 0; q < kEarlyN; ++q)
                                    if (base == q * 2 * nwaves) {  // (wave-uniform)
                                        sl[c] = el[q];
                                        ep = enp[q];
                                    }
                                if (pme != ep) sl[c] = line_of<E>(a, pme, lane & (kCandLanes - 1));
                            } else {
                                sl[c] = line_of<E>(a, pme, lane & (kCandLanes - 1));
                            }
                        }
                    }
                    bstamp(1);
#pragma unroll
                    for (int c = 0; c < kBlockDepth; ++c) {
                        const int n0 = base + c * 2 * nwaves + 2 * wv;
                        if (E::kCand) rr[c] = cand_gather2(sl[c], n0 < K, n0 + 1 < K, src);
                    }
                    bstamp(2);
#pragma unroll
                    for (int c = 0; c < kBlockDepth; ++c) {
                        const int n0 = base + c * 2 * nwaves + 2 * wv;
                        if (n0 >= K) continue;  // wave-uniform
                        // lane-wise (device_common.hpp: cand_eval2_lane): the lane that holds a half's winning candidate
                        // forms the bid and the hit test and publishes the slot's result from its own registers -- its
                        // column, and the owner and the owner's row start of its gathered record -- both halves in the
                        // same LDS instructions
                        LaneBid2 w;
                        w.hit = false;
                        w.hm = 0ull;
                        w.len[0] = w.len[1] = 0;
                        if (E::kCand) cand_eval2_lane(sl[c], rr[c], true, n0 + 1 < K, eps, w, st.bad_hi);
                        if (early && c == 0 && base < early_sweeps * 2 * nwaves) {  // (wave-uniform) the next lines of my two slots
                            int o = -2;
                            const bool both = a.cand != nullptr && __popcll(w.hm) == 2;
                            if (both) {
                                const int o0 = __builtin_amdgcn_readlane(rr[c].owner, __ffs((int)(unsigned)w.hm) - 1);
                                const int o1 = __builtin_amdgcn_readlane(rr[c].owner, __ffs((int)(unsigned)(w.hm >> 32)) + (kCandLanes - 1));
                                o = lane < kCandLanes ? o0 : o1;
                            }
#pragma unroll
                            for (int q = 0; q < kEarlyN; ++q)
                                if (base == q * 2 * nwaves) {  // (wave-uniform)
                                    if (both) el[q] = line_of<E>(a, o, lane & (kCandLanes - 1));
                                    enp[q] = o >= 0 ? o : -2;  // (an unowned object: the chain ends, the slot goes to nobody)
                                }
                        }
                        if (w.hit) {
                            const int n = n0 + (lane >> 5);
                            sKey[n] = bid_to_key(w.bid);
                            sObj[n] = sl[c].x;
                            // owner at the start of the round == what the assignment phase reads (:401): the record of
                            // obj is only rewritten by this round's winner of obj, after every bid has been made.
                            sPrev[n] = rr[c].owner;
                            sPst[n] = rr[c].ostart;
                            sHit[n] = rtag;  // (the scan pass never writes it: the slot's clean test is thread n's)
                        }
                        if (__popcll(w.hm) == 2) {  // wave-uniform (at most one lane per half): both lines decided
                            st.edges += (unsigned long long)(w.len[0] + w.len[1]);
                            st.bids += 2;
                        } else {  // a line did not decide (its slot is queued for the scan pass), or the last pair of an
                                  // odd K: its second half holds nobody
                            const bool h0 = (unsigned)w.hm != 0u, h1 = (unsigned)(w.hm >> 32) != 0u;
                            if (h0) {
                                st.edges += (unsigned long long)w.len[0];
                                st.bids += 1;
                            } else if (lane == 0) {
                                sList[atomicAdd(&sMissCnt, 1)] = n0;
                            }
                            if (n0 + 1 < K) {
                                if (h1) {
                                    st.edges += (unsigned long long)w.len[1];
                                    st.bids += 1;
                                } else if (lane == 0) {
                                    sList[atomicAdd(&sMissCnt, 1)] = n0 + 1;
                                }
                            }
                        }
                    }
#ifdef MISSLAP_TAIL_STAMP_BLOCK
                    bstamp.light(3);  // (a sweep's evaluation is billed to [8], not to the next sweep's "lines landed")
#endif
                }
                // (early: LDS-only barriers around the scan pass, so that the requested lines stay in flight.  Pass A
                // stores nothing to memory; the scan pass stores rebuilt lines, which nobody reads before the closing
                // barrier; and every record gather of the round has landed before its wavefront published the bid.)
                if (early) tail_barrier_lds();
                else __syncthreads();
                bstamp(3);
                // the clean test of the slots that pass A published, by the threads = slots (three wavefronts at K = 192,
                // next to the scan pass: inside the sweeps it would cost every wavefront a divergent loop per sweep, and
                // the registers of one -- the 1024-thread kernels then spill); a scanned slot's is its scanner's
                // (the three LDS reads are issued together: one LDS latency in front of the insert, not three)
                if (t < K) {
                    const int ts = slot_index_here(t);
                    const unsigned hit_t = sHit[ts];
                    int obj_t = sObj[ts], prev_t = sPrev[ts];
                    lds_landed_here(obj_t, prev_t);
                    if (hit_t == rtag && (clean_insert(cTab, rtag, obj_t) || prev_t < 0)) sDirty = rtag;
                }
                const int nmiss = sMissCnt;
                for (int m = wave; m < nmiss; m += nwaves) {
                    const int n = __builtin_amdgcn_readfirstlane(sList[m]);
                    const int i = __builtin_amdgcn_readfirstlane(sU[n]);
                    const int s0 = __builtin_amdgcn_readfirstlane(sStart[n]);
                    CandBid bm;
                    CandBuildArgs ba;
                    tail_scan(a, ed, s0, a.row_ptr[i + 1 + lane_zero()], eps, bm, ba, st);
                    ba.want = ba.want && a.cand != nullptr;
                    if (lane == 0) {
                        sKey[n] = bm.key;
                        sObj[n] = bm.obj;
                        sPrev[n] = bm.prev;
                        sPst[n] = bm.pstart;
                    }
                    st.edges += (unsigned long long)bm.len;
                    st.bids += 1;
                    if (ba.want) tail_build(a, i, ba, eps, st);
                    // the scanned slot's clean test (behind the rebuild: what the rebuild holds in registers is dead here)
                    if (lane == 0 && (clean_insert(cTab, rtag, bm.obj) || bm.prev < 0)) sDirty = rtag;
                }
            }
            if (early) tail_barrier_lds();
            else __syncthreads();
            bstamp(4);

            // the dirty word (one broadcast LDS read) and, in the same LDS latency, what the clean finish of slot t needs
            const int dirty = (int)sDirty;
            const int tf = slot_index_here(min(t, kTailMax - 1));
            int fu = -1, fs = 0, fo = 0, fp = 0, fq = 0;
            unsigned long long fk = 0ull;
            if (t < K) {  // (the wavefronts without a slot read the dirty word alone)
                fu = sU[tf], fs = sStart[tf], fo = sObj[tf], fp = sPrev[tf], fq = sPst[tf];
                fk = sKey[tf];
                lds_landed_here(fu, fs);
            }
            const bool clean = (unsigned)__builtin_amdgcn_readfirstlane(dirty) != rtag;
            if (clean) {
                // ---- clean round: every bidder wins (:375-385 has nothing to resolve); ASSIGN (:396-418) of slot t by
                // thread t, the slot passes to the owner its bidder evicts (:409); K and the list's order stay ----------
                if (t < K) {
                    sU[tf] = apply_winner(a, fu, fs, fo, fp, fk);
                    sStart[tf] = fq;
                }
                if (t == 0) sMissCnt = 0;
                nclean += 1ull;
            } else if (K <= kWave) {
                // ---- fast path: the whole rest of the round in wavefront 0, no LDS atomics ------------
                if (wave == 0) {
                    const bool act = lane < K;
                    const int ln = slot_index_here(lane);
                    const unsigned long long key = act ? sKey[ln] : 0ull;
                    const int obj = act ? sObj[ln] : (-2 - lane);
                    // RESOLVE (:375-385).  Two bidders on one object are the exception: every bidder inserts its object
                    // into the (empty) LDS hash table with one compare-and-swap; only if some insert meets its own object
                    // -- a contested object -- is the all-pairs loop run.  The table is emptied again right away.
                    int hs = 0;
                    bool dup = false;
                    if (act) {
                        hs = (int)(((unsigned)obj * 2654435761u) >> 21) & (kHashSize - 1);
                        for (;;) {
                            const int old = atomicCAS(&hObj[hs], -1, obj);
                            if (old == -1) break;
                            if (old == obj) {
                                dup = true;
                                break;
                            }
                            hs = (hs + 1) & (kHashSize - 1);
                        }
                    }
                    const bool contested = __any(dup);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    if (act && !dup) hObj[hs] = -1;
                    const bool lose = contested && lanes_lose(obj, key, K, lane);
                    int u = act ? sU[ln] : -1;
                    int sx = act ? sStart[ln] : 0;  // row start travelling with the slot's person
                    if (act && !lose) {
                        u = apply_winner(a, u, sx, obj, sPrev[ln], key);
                        sx = sPst[ln];
                    }
                    // push_all_left with ballots
                    const unsigned long long kmask = (K >= 64) ? ~0ull : ((1ull << K) - 1ull);
                    const unsigned long long holes = __ballot(act && u == -1) & kmask;
                    const int Kn = K - __popcll(holes);
                    const unsigned long long lmask = (Kn >= 64) ? ~0ull : ((1ull << Kn) - 1ull);
                    const unsigned long long hl = holes & lmask;            // empty slots left of K'
                    if (hl == 0ull) {  // wave-uniform: nothing to move (no hole, or only holes at the end)
                        if (act) {
                            sU[ln] = (lane < Kn) ? u : -1;
                            sStart[ln] = sx;
                        }
                    } else {
                        const unsigned long long mv = ~holes & ~lmask & kmask;  // persons right of K'
                        const bool is_hl = (hl >> lane) & 1ull, is_mv = (mv >> lane) & 1ull;
                        if (is_hl) sList[__popcll(hl & lanemask_lt())] = lane;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        if (is_mv) {
                            const int dst = sList[__popcll(mv & lanemask_lt())];
                            sU[dst] = u;
                            sStart[dst] = sx;
                        }
                        if (act) {
                            if (lane >= Kn) sU[ln] = -1;
                            else if (!is_hl) {
                                sU[ln] = u;
                                sStart[ln] = sx;
                            }
                        }
                    }
                    if (lane == 0) {
                        sK = Kn;
                        sMissCnt = 0;
                    }
                }
            } else {
                // ---- general path (64 < K <= 512): LDS hash table keyed by object ---------------------
                for (int h = t; h < kHashSize; h += kThreads) hKey[h] = 0ull;  // (it has held the clean table)
                __syncthreads();
                const bool act = t < K;
                const int tn = slot_index_here(t);
                unsigned long long key = 0ull;
                int obj = -1, h = 0;
                if (act) {
                    key = sKey[tn];
                    obj = sObj[tn];
                    h = (int)(((unsigned)obj * 2654435761u) >> 21) & (kHashSize - 1);
                    for (;;) {
                        const int old = atomicCAS(&hObj[h], -1, obj);
                        if (old == -1 || old == obj) break;
                        h = (h + 1) & (kHashSize - 1);
                    }
                    atomicMax(&hKey[h], key);
                }
                __syncthreads();
                if (act && hKey[h] == key) atomicMin(&hPos[h], t);
                __syncthreads();
                const bool win = act && hPos[h] == t;
                __syncthreads();
                if (act) {  // several threads may clear one slot: identical values
                    hObj[h] = -1;
                    hKey[h] = 0ull;
                    hPos[h] = kPosNone;
                }
                int u = act ? sU[tn] : -1;
                int sx = act ? sStart[tn] : 0;
                if (win) {
                    u = apply_winner(a, u, sx, obj, sPrev[tn], key);
                    sx = sPst[tn];
                }
                const bool hole = act && u == -1;
                const unsigned long long bh = __ballot(hole);
                if (lane == 0) sCnt[0][wave] = __popcll(bh);
                __syncthreads();
                int total = 0;
                for (int w2 = 0; w2 < nwaves; ++w2) total += sCnt[0][w2];
                const int Kn = K - total;
                const bool is_hl = hole && t < Kn;
                const bool is_mv = act && !hole && t >= Kn;
                const unsigned long long bl = __ballot(is_hl), bm = __ballot(is_mv);
                if (lane == 0) {
                    sCnt[1][wave] = __popcll(bl);
                    sCnt[2][wave] = __popcll(bm);
                }
                __syncthreads();
                int pl = __popcll(bl & lanemask_lt()), pm = __popcll(bm & lanemask_lt());
                for (int w2 = 0; w2 < wave; ++w2) {
                    pl += sCnt[1][w2];
                    pm += sCnt[2][w2];
                }
                if (is_hl) sList[pl] = t;
                __syncthreads();
                if (is_mv) {
                    sU[sList[pm]] = u;
                    sStart[sList[pm]] = sx;
                }
                if (act) {
                    if (t >= Kn) sU[tn] = -1;
                    else if (!is_hl) {
                        sU[tn] = u;
                        sStart[tn] = sx;
                    }
                }
                if (t == 0) {
                    sK = Kn;
                    sMissCnt = 0;
                }
            }
            bstamp(5);
            __syncthreads();
            bstamp(6);
            if (!clean) K = sK;
            nits += 1;
            r.mode_end(2);
            if (K == 0 || nits >= max_iter) break;
        }
#ifdef MISSLAP_TAIL_STAMP_BLOCK
        if (t == 0)
            for (int k = 1; k <= 6; ++k) a.ctl->dbg[5 + k] += bacc[k];
#endif
#if !defined(MISSLAP_TAIL_STAMP) && !defined(MISSLAP_TAIL_STAMP_SOLO) && !defined(MISSLAP_TAIL_STAMP_DUO) && \
    !defined(MISSLAP_TAIL_STAMP_TEAM) && !defined(MISSLAP_TAIL_STAMP_BLOCK) && !defined(MISSLAP_TILED_STAMP)
        if (t == 0) a.ctl->dbg[6] += nclean;  // (the stamped builds use the slot for a segment)
#endif
    }
};

// ---- the four kernels: entry tests and list (tail_begin), the role's LDS, its modes, tail_end ------------------------------
// K > kTeamMax.  Block rounds have the most bidders, i.e. spend the most lines: a quarter of a launch's round budget.
template <class E>
struct k_tail_block {
    MISSLAP_KERNEL(2 * kTailMax)
    static __device__ __forceinline__ void run(TailArgs a, E ed) {
        __shared__ int sU[kTailMax];
        __shared__ int sStart[kTailMax];  // row start of the person in slot n, kept next to sU: evicted owners bring
                                          // theirs with the price record, so no row_ptr load precedes a row fetch
        TailRun r;
        const int budget = a.round_budget > 0 ? max(a.round_budget / 4, 1) : 0;
        if (!tail_begin(a, budget, kTeamMax + 1, kTailMax, sU, sStart, kTailMax, kBlock, r)) return;
        tail_block_mode<E, kBlock>::run(a, ed, sU, sStart, r, E::kCand ? kEarlySweeps : 0);  // (opens with a barrier)
        tail_end(a, sU, kBlock, r);
    }
};

// 3 <= K <= kTeamMax, handles with lines: one list slot per wavefront
template <class E>
struct k_tail_team {
    MISSLAP_KERNEL(2 * kTailMax)
    static_assert(kBlock / kWave == kTeamMax, "one slot per wavefront");
    static __device__ __forceinline__ void run(TailArgs a, E ed) {
        __shared__ int sU[kTeamMax];
        __shared__ int sStart[kTeamMax];
        TailRun r;
        if (!tail_begin(a, a.round_budget, 3, kTeamMax, sU, sStart, kTeamMax, kBlock, r)) return;
        __syncthreads();
        r.mode_begin(1);
        if (tail_team1_pipe(a, ed, sU, sStart, r.K, r.nits, r.max_iter, r.eps, r.st)) {
            tail_flush_stats(a.ctl, r.st);  // this wavefront's slot fell away: it ends here, with its statistics
            return;
        }
        r.mode_end(1);
        tail_end(a, sU, kBlock, r);
    }
};

// K <= 2, handles with lines: one wavefront, pair rounds while two bidders are left, then the chain
template <class E>
struct k_tail_pair {
    MISSLAP_KERNEL(kWave)
    static __device__ __forceinline__ void run(TailArgs a, E ed) {
        __shared__ int sU[2];
        __shared__ int sStart[2];
        TailRun r;
        if (!E::kCand || a.cand == nullptr) return;  // no lines: k_tail_nolines' rounds
        if (!tail_begin(a, a.round_budget, 1, 2, sU, sStart, 2, kBlock, r)) return;
        __syncthreads();
        r.mode_begin(0);
        tail_pair_mode(a, ed, sU, sStart, r.K, r.nits, r.max_iter, r.eps, r.st);
        r.mode_end(0);  // K == 0 or nits == max_iter
        tail_end(a, sU, kBlock, r);
    }
};

// Every K, for a handle whose lines are switched off (launched for no other): block -> team -> solo / chain.  The team
// and solo modes of this kernel need more than the 128 registers a 1024-thread workgroup leaves a wavefront.
template <class E>
struct k_tail_nolines {
    MISSLAP_KERNEL(kTailMax)
    static __device__ __forceinline__ void run(TailArgs a, E ed) {
        __shared__ int sU[kTailMax];
        __shared__ int sStart[kTailMax];
        __shared__ int sK;
        __shared__ long long sNits;
        TailRun r;
        if (!tail_begin(a, a.round_budget, 1, kTailMax, sU, sStart, kTailMax, kBlock, r)) return;
        __syncthreads();
        if (r.K > kTeamMax) tail_block_mode<E, kBlock>::run(a, ed, sU, sStart, r, 0);
        if (r.K > 2 && r.nits < r.max_iter) {  // every wavefront, until K <= 2 (or max_iter)
            r.mode_begin(1);
            tail_team_mode(a, ed, sU, sStart, r.K, r.nits, r.max_iter, r.eps, r.st);
            r.mode_end(1);
        }
        if (r.K > 0 && r.nits < r.max_iter) {  // K <= 2: wavefront 0 runs the rest of the phase alone
            if (threadIdx.x < kWave) {
                r.mode_begin(0);
                tail_solo_mode(a, ed, sU, sStart, r.K, r.nits, r.max_iter, r.eps, r.st);
                r.mode_end(0);
                if (threadIdx.x == 0) sK = r.K, sNits = r.nits;
            }
            __syncthreads();
            r.K = sK;
            r.nits = sNits;
        }
        tail_end(a, sU, kBlock, r);
    }
};

}  // namespace misslap
