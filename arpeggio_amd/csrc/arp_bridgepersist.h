// arp_bridgepersist.h — water-bridge persistence over the models of an ensemble, reduced on the device.
//
// The bridge table of arp_bridge.h over the F resident models, folded per pair of TOPOLOGY atoms — or of topology residues
// (ARP_WBP_BY_RESIDUE) —: in how many models a water bridges the pair, through how many waters, with which SIFt bits on either
// leg, and how tight the bridge is (its path, dist_a + dist_b as one float32 addition).  Its size does not depend on F, so only
// the table crosses PCIe.
//
// Shape (that of arp_respersist.h):
//   k_bridgepersist_rekey      one thread per bridge row (w, a, b): model f = w / n, key pair_lo << (bits + fbits) |
//                              pair_hi << fbits | f, payload the row's index | swapped << 32.  At atom level the pair is
//                              (a - f n, b - f n), already ascending; at residue level the topology residues of a and b, min
//                              first, and `swapped` says that leg b is the one whose partner lies in res_a.  The nine columns
//                              of a row do not fit a payload: the reduction gathers them by the index.
//   (radix passes of arp_sort.h over every bit of the key)
//   k_runs_count / k_runs_scan / k_runs_starts (arp_runs.h, shift fbits): a run = one pair; U = rows
//   k_bridgepersist_reduce     one wave per row, 64 consecutive sorted records per step
// Every bridge row has a row of the table: no record is left out, so the records of a run are exactly [row_start[r],
// row_start[r + 1]).
//
// A run holds several records per model (several waters for one pair, and at residue level several atom pairs for one water),
// ascending by f.  "Models with property X" is a count of SEGMENTS of equal f, found as k_respersist_reduce finds them; the
// model that is still open at the end of a step travels to the next one as wave-uniform state.  The distinct waters of a model
// rely on the order INSIDE a segment: the least-significant-digit sort is stable, the bridge table ascends by (water, a, b)
// and the re-key keeps that order, so the records of one (pair, model) still ascend by water.  A water id is a resident id —
// it names its model —, so a record begins a new water exactly where `water` differs from the record before it in the run, in
// or across segments; the last water seen travels across the 64-step carry beside the open model.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_runs.h"

#define BRIDGEPERSIST_BY_RESIDUE 2u      // ARP_WBP_BY_RESIDUE
// lanes of k_bridgepersist_reduce that keep a count: b < 15 SIFt bit b of leg a, 15 + b of leg b, then the models and the waters
#define BRIDGEPERSIST_LANE_MODELS (2 * TABLE_SIFT_BITS)
#define BRIDGEPERSIST_LANE_WATERS (BRIDGEPERSIST_LANE_MODELS + 1)
#define BRIDGEPERSIST_SWAPPED (1ull << 32)

struct BridgepersistArgs {
    int bits, fbits;         // key = pair_lo << (bits + fbits) | pair_hi << fbits | f
    uint32_t n, nres_t;      // atoms / residues of one model
    uint32_t flags;          // ARP_WBP_BY_RESIDUE
    // the bridge table (BRIDGE_TABLE), rows ascending by (water, a, b)
    const int* b_w;
    const int* b_a;
    const int* b_b;
    const float* b_da;
    const float* b_db;
    const uint16_t* b_sa;
    const uint16_t* b_sb;
    const uint8_t* b_ca;
    const uint8_t* b_cb;
    long long rows;          // B
    const int* res_id;       // per resident atom
    // the re-keyed rows: written by k_bridgepersist_rekey, read sorted by k_bridgepersist_reduce
    unsigned long long* key;
    unsigned long long* val;
    const int* row_start;    // [U + 1] (RunArgs)
    long long U;
    // the table, one column after the other (BRIDGEPERSIST_TABLE)
    int* t_a;
    int* t_b;
    uint16_t* t_nmodels;
    int* t_first;
    int* t_last;
    uint32_t* t_nwaters;
    uint32_t* t_nbridges;
    float* t_dmin;
    float* t_dmax;
    double* t_dsum;
    uint16_t* t_bits_a;      // [U][TABLE_SIFT_BITS]
    uint16_t* t_bits_b;
    uint8_t* t_ctype_a;
    uint8_t* t_ctype_b;
};

__global__ __launch_bounds__(256) void k_bridgepersist_rekey(BridgepersistArgs A) {
    const bool by_res = (A.flags & BRIDGEPERSIST_BY_RESIDUE) != 0;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < A.rows; r += (long long)gridDim.x * blockDim.x) {
        const uint32_t a = (uint32_t)A.b_a[r], b = (uint32_t)A.b_b[r];
        const uint32_t f = (uint32_t)A.b_w[r] / A.n;
        uint32_t lo, hi;
        unsigned long long v = (unsigned long long)r;
        if (by_res) {
            const uint32_t ra = (uint32_t)A.res_id[a] - f * A.nres_t, rb = (uint32_t)A.res_id[b] - f * A.nres_t;
            lo = ra < rb ? ra : rb;
            hi = ra < rb ? rb : ra;
            if (ra > rb) v |= BRIDGEPERSIST_SWAPPED;
        } else {
            lo = a - f * A.n;
            hi = b - f * A.n;
        }
        A.key[r] = ((unsigned long long)lo << (A.bits + A.fbits)) | ((unsigned long long)hi << A.fbits) | (unsigned long long)f;
        A.val[r] = v;
    }
}

// What a closed model adds to dist_min / dist_max / dist_sum, on every lane alike: its smallest path.
struct BridgepersistRow {
    uint32_t cnt;
    float dmin, dmax;
    double dsum;
};
__device__ __forceinline__ void bridgepersist_close(BridgepersistRow& r, int lane, uint32_t sa, uint32_t sb, float m) {
    if (lane < TABLE_SIFT_BITS) r.cnt += (sa >> lane) & 1u;
    else if (lane < BRIDGEPERSIST_LANE_MODELS) r.cnt += (sb >> (lane - TABLE_SIFT_BITS)) & 1u;
    else if (lane == BRIDGEPERSIST_LANE_MODELS) r.cnt += 1u;
    r.dmin = m < r.dmin ? m : r.dmin;
    r.dmax = m > r.dmax ? m : r.dmax;
    r.dsum += (double)m;
}

__global__ __launch_bounds__(256) void k_bridgepersist_reduce(BridgepersistArgs A) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const unsigned long long fmask = (1ull << A.fbits) - 1ull, pmask = (1ull << A.bits) - 1ull;
    const float inf = __uint_as_float(0x7F800000u);
    for (long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < A.U; row += waves) {
        const long long s = A.row_start[row], e = A.row_start[row + 1];
        const unsigned long long k0 = A.key[s];
        BridgepersistRow r{0u, inf, -inf, 0.0};
        uint32_t types_a = 0, types_b = 0;
        // the open model: wave-uniform.  Its f, the last water seen, the OR of either leg's SIFt, its smallest path
        bool open = false;
        uint32_t c_f = 0, c_sa = 0, c_sb = 0;
        int c_w = -1;
        float c_min = inf;
        for (long long q = s; q < e; q += 64) {      // (wave-uniform trip count)
            const bool valid = q + lane < e;
            const int nv = (int)min((long long)64, e - q);
            uint32_t f = 0, sa = 0, sb = 0;
            int w = -1;
            float d = inf;
            if (valid) {
                const unsigned long long v = A.val[q + lane];
                const long long at = (long long)(v & 0xFFFFFFFFull);      // (at < B: the payload is the row's index)
                f = (uint32_t)(A.key[q + lane] & fmask);
                w = A.b_w[at];
                d = A.b_da[at] + A.b_db[at];         // the path: one float32 addition, which commutes — the leg order cannot show
                sa = A.b_sa[at]; sb = A.b_sb[at];
                uint32_t ca = A.b_ca[at], cb = A.b_cb[at];
                if (v & BRIDGEPERSIST_SWAPPED) {
                    const uint32_t ts = sa, tc = ca;
                    sa = sb; sb = ts;
                    ca = cb; cb = tc;
                }
                sa &= 0x7FFFu; sb &= 0x7FFFu;
                types_a |= 1u << (ca & 7u);
                types_b |= 1u << (cb & 7u);
            }
            // ---- segments: a lane is a head when its f differs from the lane before (lane 0: from the open model); a water
            // begins where the water differs from the record before (lane 0: from the last water of the step before)
            const uint32_t fp = __shfl_up(f, 1);
            const int wp = __shfl_up(w, 1);
            const bool head = valid && (lane == 0 ? (!open || f != c_f) : f != fp);
            const bool water = valid && (lane == 0 ? (!open || w != c_w) : w != wp);
            const unsigned long long hb = __ballot(head);
            const bool cont = open && !(hb & 1ull);          // the open model goes on in this step's first segment
            if (open && !cont) bridgepersist_close(r, lane, c_sa, c_sb, c_min);      // ... or it is closed before this step's models
            const unsigned long long starts = hb | 1ull;
            const int start = 63 - __clzll(starts & (~0ull >> (63 - lane)));
            const unsigned long long above = starts & ~((2ull << lane) - 1ull);
            const int end = above ? __ffsll((long long)above) - 1 : nv;
            const unsigned long long below_end = end >= 64 ? ~0ull : (1ull << end) - 1ull;
            const unsigned long long seg = end > start ? below_end & ~((1ull << start) - 1ull) : 0ull;
            const bool carried = cont && start == 0;         // this lane's segment is the open model's
            const bool closing = valid && lane == end - 1 && end < nv;      // a model ends inside this step: every segment but the last
            // ---- per-model presence: each ballot of the step restricted to the lane's own segment, and counted where a model ends
            uint32_t m_sa = carried ? c_sa : 0u, m_sb = carried ? c_sb : 0u;
#pragma unroll
            for (int b = 0; b < TABLE_SIFT_BITS; ++b) {
                m_sa |= (__ballot((sa >> b) & 1u) & seg) ? 1u << b : 0u;
                m_sb |= (__ballot((sb >> b) & 1u) & seg) ? 1u << b : 0u;
                const uint32_t na = (uint32_t)__popcll(__ballot(closing && ((m_sa >> b) & 1u)));
                const uint32_t nb = (uint32_t)__popcll(__ballot(closing && ((m_sb >> b) & 1u)));
                if (lane == b) r.cnt += na;
                if (lane == TABLE_SIFT_BITS + b) r.cnt += nb;
            }
            {
                const uint32_t c = (uint32_t)__popcll(__ballot(closing)), nw = (uint32_t)__popcll(__ballot(water));
                if (lane == BRIDGEPERSIST_LANE_MODELS) r.cnt += c;
                if (lane == BRIDGEPERSIST_LANE_WATERS) r.cnt += nw;
            }
            // ---- per-model minimum: an inclusive scan that stops at segment heads; the segment's last lane holds the minimum
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float t = __shfl_up(d, o);
                if (lane - o >= start) d = t < d ? t : d;
            }
            if (carried) d = c_min < d ? c_min : d;
            // their smallest paths one by one in lane order (= ascending model): every lane keeps the same sum
            for (unsigned long long cm = __ballot(closing); cm; cm &= cm - 1ull) {
                const float m = __shfl(d, __ffsll((long long)cm) - 1);
                r.dmin = m < r.dmin ? m : r.dmin;
                r.dmax = m > r.dmax ? m : r.dmax;
                r.dsum += (double)m;
            }
            // ---- the step's last segment stays open
            open = true;
            c_f = __shfl(f, nv - 1);
            c_w = __shfl(w, nv - 1);
            c_sa = __shfl(m_sa, nv - 1);
            c_sb = __shfl(m_sb, nv - 1);
            c_min = __shfl(d, nv - 1);
        }
        // the run ends: its last model closes (a run has a record, so there is one)
        if (open) bridgepersist_close(r, lane, c_sa, c_sb, c_min);
        for (int o = 32; o > 0; o >>= 1) {
            types_a |= __shfl_xor(types_a, o);
            types_b |= __shfl_xor(types_b, o);
        }
        if (lane < TABLE_SIFT_BITS) A.t_bits_a[row * TABLE_SIFT_BITS + lane] = (uint16_t)r.cnt;
        else if (lane < BRIDGEPERSIST_LANE_MODELS) A.t_bits_b[row * TABLE_SIFT_BITS + (lane - TABLE_SIFT_BITS)] = (uint16_t)r.cnt;
        else if (lane == BRIDGEPERSIST_LANE_MODELS) A.t_nmodels[row] = (uint16_t)r.cnt;
        else if (lane == BRIDGEPERSIST_LANE_WATERS) A.t_nwaters[row] = r.cnt;
        if (lane == 0) {
            A.t_a[row] = (int)(k0 >> (A.bits + A.fbits));
            A.t_b[row] = (int)((k0 >> A.fbits) & pmask);
            A.t_first[row] = (int)(k0 & fmask);
            A.t_last[row] = (int)c_f;
            A.t_nbridges[row] = (uint32_t)(e - s);
            A.t_dmin[row] = r.dmin;
            A.t_dmax[row] = r.dmax;
            A.t_dsum[row] = r.dsum;
            A.t_ctype_a[row] = (uint8_t)types_a;
            A.t_ctype_b[row] = (uint8_t)types_b;
        }
    }
}
