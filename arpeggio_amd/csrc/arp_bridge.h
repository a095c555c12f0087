// arp_bridge.h — water-mediated contacts: the atom-atom bag of a pass joined with itself on its water atoms, on the device
// (DESIGN.md 5i).  A LEG is a record with exactly one water atom (ARP_F_WATER) and a wanted SIFt bit; the water is w, the
// other atom the partner.  A BRIDGE is a water w with an unordered pair of its partners a < b — one row (w, a, b) that carries
// both legs' distance, SIFt and contact type —, dropped when a and b share a residue unless ARP_WB_SAME_RESIDUE is given.
// Rows ascend by (w, a, b).  Unlike the filter (5h) and the folds (5e - 5g) a row comes from TWO records, and there are more
// rows than legs.  No atomics on global memory, no look-back, no block waits for another, plain stores:
//   k_bridge_legs_count  block t: legs of tile t (the tiling of k_filter_count)                          -> tile_keep[t]
//   k_runs_scan          (arp_runs.h, one block) exclusive prefix of those counts; their sum L = legs
//   (the host reads L — wait 1 — and sizes everything below by it)
//   k_bridge_legs_write  block t: key w << pbits | partner and payload table_payload(dist, sift, ctype, 0) of its legs at
//                        tile_keep[t] + rank in the tile
//   (radix passes of arp_sort.h over every bit of the key: a water's legs are then one run, partners ascending)
//   k_runs_count / k_runs_scan / k_runs_starts (arp_runs.h, shift pbits): U = waters with a leg stays on the device —
//                        row_start is sized for L runs, and the kernels below read U from where k_runs_scan left it
//   k_bridge_leg_res     leg_res[p] = res_id[partner of sorted leg p]: a residue is read once per leg, never per pair
//                        (not launched under ARP_WB_SAME_RESIDUE)
//   k_bridge_pairs<false>  one wave per run: its kept pairs, 64-bit                                      -> row_off[r]
//   k_bridge_scan        one block: exclusive 64-bit prefix of those counts in place; row_off[L] = B = rows
//   (the host reads B — wait 2 — and sizes the nine columns)
//   k_bridge_pairs<true>   the same walk; pair (p, q) of a run is written at row_off[r] + its rank among the run's kept
//                        pairs in (p, q) order, so the rows come out in the contract's order and nothing sorts them
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_filter.h"

#define BRIDGE_F_WATER 4u        // ARP_F_WATER
#define BRIDGE_SAME_RESIDUE 1u   // ARP_WB_SAME_RESIDUE

struct BridgeLegArgs {
    // the bag of the pass, unsorted
    const int* ci;
    const int* cj;
    const float* d_in;
    const uint16_t* s_in;
    const uint8_t* ct_in;
    long long k;             // records
    const uint16_t* flags;   // per atom
    uint32_t sift_any;       // low 15 bits
    int pbits;               // key = w << pbits | partner
    int* tile_keep;          // [T]: legs of tile t, then (k_runs_scan) their exclusive prefix
    unsigned long long* key; // [L] (k_bridge_legs_write)
    unsigned long long* val;
    long long legs;          // L
};

struct BridgePairArgs {
    // the legs, sorted by (w, partner)
    const unsigned long long* key;
    const unsigned long long* val;
    long long legs;          // L
    int pbits;
    const int* row_start;    // [U] first leg of run r (k_runs_starts made it for L runs: row_start[U] is NOT the end of the last)
    const long long* runs;   // [1]: U, as k_runs_scan left it
    const int* res_id;       // per atom
    int* leg_res;            // [L] residue of the partner of leg p
    uint32_t flags;          // ARP_WB_*
    long long* row_off;      // [L + 1]: kept pairs of run r, then their exclusive prefix; row_off[L] = B
    long long rows;          // B
    // the table, one column after the other (BRIDGE_TABLE)
    int* t_w;
    int* t_a;
    int* t_b;
    float* t_da;
    float* t_db;
    uint16_t* t_sa;
    uint16_t* t_sb;
    uint8_t* t_ca;
    uint8_t* t_cb;
};

// Bit r of the result: record lo + r of the thread's FILTER_ITEMS consecutive records is a leg; then w[r] / pa[r] are its
// water and its partner.  The SIFt test comes first (filter_keep's loads, every contact type let through): the atoms and
// their flags are read for the records that pass it only.
__device__ __forceinline__ uint32_t bridge_legs(const BridgeLegArgs& A, long long lo, uint32_t sf[FILTER_ITEMS], uint32_t ct[FILTER_ITEMS],
                                                int w[FILTER_ITEMS], int pa[FILTER_ITEMS]) {
    FilterArgs F{};
    F.s_in = A.s_in; F.ct_in = A.ct_in; F.k = A.k; F.sift_any = A.sift_any; F.ctype_mask = (1u << FILTER_CTYPES) - 1u;
    uint32_t m = filter_keep(F, lo, sf, ct);
#pragma unroll
    for (int r = 0; r < FILTER_ITEMS; ++r) {
        w[r] = pa[r] = 0;
        if ((m >> r) & 1u) {
            const int i = A.ci[lo + r], j = A.cj[lo + r];
            const bool wi = (A.flags[i] & BRIDGE_F_WATER) != 0, wj = (A.flags[j] & BRIDGE_F_WATER) != 0;
            if (wi != wj) { w[r] = wi ? i : j; pa[r] = wi ? j : i; }
            else m &= ~(1u << r);
        }
    }
    return m;
}

__global__ __launch_bounds__(FILTER_THREADS) void k_bridge_legs_count(BridgeLegArgs A) {
    __shared__ int s_w[FILTER_THREADS / 64];
    uint32_t sf[FILTER_ITEMS], ct[FILTER_ITEMS];
    int w[FILTER_ITEMS], pa[FILTER_ITEMS];
    int c = __popc(bridge_legs(A, (long long)blockIdx.x * FILTER_TILE + (long long)threadIdx.x * FILTER_ITEMS, sf, ct, w, pa));
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int v = 0; v < FILTER_THREADS / 64; ++v) t += s_w[v];
        A.tile_keep[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(FILTER_THREADS) void k_bridge_legs_write(BridgeLegArgs A) {
    __shared__ long long s_w[SORT_WAVES];
    static_assert(FILTER_THREADS == SORT_THREADS, "sort_block_scan scans SORT_THREADS values");
    const long long lo = (long long)blockIdx.x * FILTER_TILE + (long long)threadIdx.x * FILTER_ITEMS;
    uint32_t sf[FILTER_ITEMS], ct[FILTER_ITEMS];
    int w[FILTER_ITEMS], pa[FILTER_ITEMS];
    const uint32_t m = bridge_legs(A, lo, sf, ct, w, pa);
    long long pos = (long long)A.tile_keep[blockIdx.x] + sort_block_scan((long long)__popc(m), s_w, nullptr);
#pragma unroll
    for (int r = 0; r < FILTER_ITEMS; ++r)
        if ((m >> r) & 1u) {
            if (pos < A.legs) {      // (pos < L always: L is the sum of the same counts)
                A.key[pos] = ((unsigned long long)(uint32_t)w[r] << A.pbits) | (unsigned long long)(uint32_t)pa[r];
                A.val[pos] = table_payload(A.d_in[lo + r], sf[r], ct[r], 0ull);
            }
            ++pos;
        }
}

__global__ __launch_bounds__(256) void k_bridge_leg_res(BridgePairArgs A) {
    const unsigned long long pmask = (1ull << A.pbits) - 1ull;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < A.legs; p += (long long)gridDim.x * blockDim.x)
        A.leg_res[p] = A.res_id[(int)(A.key[p] & pmask)];
}

// The walk of one 64-step of a run: lane = leg p = p0 + lane of the run [s, s + m), against every leg q > p, 64 values of q a
// trip (wave-uniform trip counts; the legs of a trip are loaded one a lane and handed round by lane index).  A pair is kept when
// the partners' residues differ, or always under `all`.  Returns the lane's kept pairs; EMIT: writes them, ascending q, from
// row `at` on.
template <bool EMIT>
__device__ __forceinline__ long long bridge_walk(const BridgePairArgs& A, long long s, long long m, long long p0, int lane, bool all, long long at) {
    const unsigned long long pmask = (1ull << A.pbits) - 1ull;
    const long long p = p0 + lane;
    const bool mine = p < m;
    const int rp = (mine && !all) ? A.leg_res[s + p] : 0;
    if (!EMIT && all) return mine ? m - 1 - p : 0;      // (every q > p)
    unsigned long long kp = 0, vp = 0;
    if (EMIT && mine) { kp = A.key[s + p]; vp = A.val[s + p]; }
    long long n = 0;
    for (long long q0 = p0; q0 < m; q0 += 64) {
        const bool have = q0 + lane < m;
        const int rq_l = (have && !all) ? A.leg_res[s + q0 + lane] : 0;
        unsigned long long kq_l = 0, vq_l = 0;
        if (EMIT && have) { kq_l = A.key[s + q0 + lane]; vq_l = A.val[s + q0 + lane]; }
        const int trips = (int)min((long long)64, m - q0);
        for (int t = 0; t < trips; ++t) {
            const int rq = __shfl(rq_l, t);
            const bool keep = mine && q0 + t > p && (all || rq != rp);
            if (EMIT) {
                const unsigned long long kq = __shfl(kq_l, t), vq = __shfl(vq_l, t);
                if (keep && at + n < A.rows) {      // (at + n < B always: B is the sum of the same counts)
                    const long long r = at + n;
                    A.t_w[r] = (int)(kp >> A.pbits);
                    A.t_a[r] = (int)(kp & pmask);
                    A.t_b[r] = (int)(kq & pmask);
                    A.t_da[r] = payload_distance(vp);
                    A.t_db[r] = payload_distance(vq);
                    A.t_sa[r] = (uint16_t)payload_sift(vp);
                    A.t_sb[r] = (uint16_t)payload_sift(vq);
                    A.t_ca[r] = (uint8_t)payload_type(vp);
                    A.t_cb[r] = (uint8_t)payload_type(vq);
                }
            }
            n += keep ? 1 : 0;
        }
    }
    return n;
}

// One wave per water run.  WRITE = false: row_off[r] = kept pairs of run r.  WRITE = true: the rows of run r from row_off[r]
// on — the rank of pair (p, q) is the kept pairs of earlier 64-steps (carry) + those of lower lanes of this step (wave
// prefix) + those of this lane with a smaller q: the count of kept pairs before it in (p, q) order.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_bridge_pairs(BridgePairArgs A) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const long long U = min(A.runs[0], A.legs);
    const bool all = (A.flags & BRIDGE_SAME_RESIDUE) != 0;
    for (long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < U; row += waves) {
        const long long s = A.row_start[row], e = row + 1 < U ? (long long)A.row_start[row + 1] : A.legs;
        const long long m = e - s;
        long long carry = 0;
        for (long long p0 = 0; p0 < m; p0 += 64) {      // (wave-uniform trip count)
            const long long c = bridge_walk<false>(A, s, m, p0, lane, all, 0);
            long long incl = c;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const long long u = __shfl_up(incl, off);
                if (lane >= off) incl += u;
            }
            if (WRITE) (void)bridge_walk<true>(A, s, m, p0, lane, all, A.row_off[row] + carry + incl - c);
            carry += __shfl(incl, 63);
        }
        if (!WRITE && lane == 0) A.row_off[row] = carry;
    }
}

// one block (SORT_THREADS threads: sort_block_scan): exclusive prefix of the U per-run counts in place, 64-bit; their sum B
// goes to row_off[L], a slot the host knows without knowing U
__global__ __launch_bounds__(SORT_THREADS) void k_bridge_scan(BridgePairArgs A) {
    __shared__ long long s_w[SORT_WAVES];
    const long long U = min(A.runs[0], A.legs);
    long long run = 0;
    for (long long r0 = 0; r0 < U; r0 += SORT_THREADS) {      // (block-uniform trip count)
        const long long r = r0 + threadIdx.x;
        const long long v = r < U ? A.row_off[r] : 0;
        long long sum;
        const long long x = sort_block_scan(v, s_w, &sum);
        if (r < U) A.row_off[r] = run + x;
        run += sum;
    }
    if (threadIdx.x == 0) A.row_off[A.legs] = run;
}
