// arp_respersist.h — residue contact persistence over the models of an ensemble, reduced on the device.
//
// The product of the two tables before it: per pair of TOPOLOGY residues (arp_respair.h's fold by residue), over the F resident
// models (arp_persist.h's fold over the models) — in how many models the two residues touch, through which of the five record
// classes, with which SIFt bits, and how closely.  Its size does not depend on F, so only the table crosses PCIe.
//
// Shape (that of both neighbours):
//   k_residue_rekey / k_residue_rekey_planes (arp_respair.h): the records of the five bags -> key res_a << (rbits + fbits) |
//                              res_b << fbits | f (respersist_key), payload table_payload (arp_runs.h), class 0 ... 4
//   (radix passes of arp_sort.h over every bit of the key)
//   k_runs_count / k_runs_scan / k_runs_starts (arp_runs.h, shift fbits): a run = one residue pair; U = rows
//   k_respersist_reduce        one wave per row, 64 consecutive sorted records per step
// Records that are left out (a residue of -1) keep their slot with an all-ones key and class TABLE_LEFT_OUT, as in
// arp_respair.h and for its reason: they trail the last run, no run begins on them, and the host needs no second wait.
//
// What neither neighbour needed: after the sort a run holds SEVERAL records per model (every atom pair of the two residues,
// every ring / amide record), ascending by f and in arbitrary order within a model.  "Models with property X" is therefore a
// count of SEGMENTS of equal f, not of records.  k_respersist_reduce finds the segments of a step with one ballot, gives every
// lane the mask of its own segment, and evaluates each per-model quantity (an OR, a presence, a minimum) at the segment's last
// lane; the model that is still open at the end of a step travels to the next one as wave-uniform state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_respair.h"

#define RESPERSIST_CLASSES 5     // atom-atom, atom-plane, plane-plane, group-group, group-plane
// lanes of k_respersist_reduce that keep a count: b < 15 SIFt bit b, 15 + m class m, then the models and the atom-atom records
#define RESPERSIST_LANE_MODELS (TABLE_SIFT_BITS + RESPERSIST_CLASSES)
#define RESPERSIST_LANE_CONTACTS (RESPERSIST_LANE_MODELS + 1)

struct RespersistArgs {
    int rbits, fbits;        // key = res_a << (rbits + fbits) | res_b << fbits | f
    // the re-keyed records, sorted
    const unsigned long long* key;
    const unsigned long long* val;
    const int* row_start;    // [U + 1] (RunArgs)
    long long U;
    // the table, one column after the other (RESPERSIST_TABLE)
    double* t_dsum;
    int* t_a;
    int* t_b;
    int* t_first;
    int* t_last;
    uint32_t* t_n;
    float* t_dmin;
    float* t_dmax;
    uint16_t* t_nmodels;
    uint16_t* t_cls;         // [U][RESPERSIST_CLASSES]
    uint16_t* t_bits;        // [U][TABLE_SIFT_BITS]
    uint8_t* t_ctype;
};

// What a closed model adds to the row, on every lane alike: its SIFt bits and classes to the counts (lane b keeps count b),
// and — when it has an atom-atom record — its smallest distance to dist_min / dist_max / dist_sum.
struct RespersistRow {
    uint32_t cnt;
    float dmin, dmax;
    double dsum;
};
__device__ __forceinline__ void respersist_close_distance(RespersistRow& r, float m) {
    r.dmin = m < r.dmin ? m : r.dmin;
    r.dmax = m > r.dmax ? m : r.dmax;
    r.dsum += (double)m;
}

__global__ __launch_bounds__(256) void k_respersist_reduce(RespersistArgs A) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const unsigned long long fmask = (1ull << A.fbits) - 1ull, rmask = (1ull << A.rbits) - 1ull;
    const float inf = __uint_as_float(0x7F800000u);
    for (long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < A.U; row += waves) {
        // (the last row's range also holds the left-out records that trail it: invalid lanes below)
        const long long s = A.row_start[row], e = A.row_start[row + 1];
        const unsigned long long k0 = A.key[s];
        RespersistRow r{0u, inf, -inf, 0.0};
        uint32_t types = 0;
        // the open model: wave-uniform.  Its f, the OR of its SIFt bits (atom-atom records), its classes, its smallest distance
        bool open = false;
        uint32_t c_f = 0, c_sf = 0, c_cls = 0;
        float c_min = inf;
        for (long long q = s; q < e; q += 64) {      // (wave-uniform trip count)
            const bool in = q + lane < e;
            const unsigned long long v = in ? A.val[q + lane] : TABLE_LEFT_OUT << TABLE_CLASS_SHIFT;
            const uint32_t cls = payload_class(v);
            const bool valid = cls < (uint32_t)RESPERSIST_CLASSES;      // (valid lanes are a prefix: the left-out records sort last)
            const int nv = __popcll(__ballot(valid));
            if (nv == 0) break;
            const uint32_t f = valid ? (uint32_t)(A.key[q + lane] & fmask) : 0u;
            const bool aa = cls == 0u;
            const uint32_t sf = aa ? payload_sift(v) : 0u;
            if (aa) types |= 1u << payload_type(v);
            // ---- segments: a lane is a head when its f differs from the lane before (lane 0: from the open model)
            const uint32_t fp = __shfl_up(f, 1);
            const bool head = valid && (lane == 0 ? (!open || f != c_f) : f != fp);
            const unsigned long long hb = __ballot(head);
            const bool cont = open && !(hb & 1ull);          // the open model goes on in this step's first segment
            if (open && !cont) {                             // ... or it is closed before this step's models
                if (lane < TABLE_SIFT_BITS) r.cnt += (c_sf >> lane) & 1u;
                else if (lane < RESPERSIST_LANE_MODELS) r.cnt += (c_cls >> (lane - TABLE_SIFT_BITS)) & 1u;
                else if (lane == RESPERSIST_LANE_MODELS) r.cnt += 1u;
                if (c_cls & 1u) respersist_close_distance(r, c_min);
            }
            const unsigned long long starts = hb | 1ull;
            const int start = 63 - __clzll(starts & (~0ull >> (63 - lane)));
            const unsigned long long above = starts & ~((2ull << lane) - 1ull);
            const int end = above ? __ffsll((long long)above) - 1 : nv;
            const unsigned long long below_end = end >= 64 ? ~0ull : (1ull << end) - 1ull;
            const unsigned long long seg = end > start ? below_end & ~((1ull << start) - 1ull) : 0ull;
            const bool carried = cont && start == 0;         // this lane's segment is the open model's
            const bool closing = valid && lane == end - 1 && end < nv;      // a model ends inside this step: every segment but the last
            // ---- per-model presence: each ballot of the step restricted to the lane's own segment, and counted where a model ends
            uint32_t m_sf = carried ? c_sf : 0u, m_cls = carried ? c_cls : 0u;
#pragma unroll
            for (int b = 0; b < TABLE_SIFT_BITS; ++b) {
                m_sf |= (__ballot((sf >> b) & 1u) & seg) ? 1u << b : 0u;
                const uint32_t c = (uint32_t)__popcll(__ballot(closing && ((m_sf >> b) & 1u)));
                if (lane == b) r.cnt += c;
            }
#pragma unroll
            for (int m = 0; m < RESPERSIST_CLASSES; ++m) {
                m_cls |= (__ballot(cls == (uint32_t)m) & seg) ? 1u << m : 0u;
                const uint32_t c = (uint32_t)__popcll(__ballot(closing && ((m_cls >> m) & 1u)));
                if (lane == TABLE_SIFT_BITS + m) r.cnt += c;
            }
            {
                const uint32_t c = (uint32_t)__popcll(__ballot(closing)), n = (uint32_t)__popcll(__ballot(aa));
                if (lane == RESPERSIST_LANE_MODELS) r.cnt += c;
                if (lane == RESPERSIST_LANE_CONTACTS) r.cnt += n;
            }
            // ---- per-model minimum: an inclusive scan that stops at segment heads; the segment's last lane holds the minimum
            float d = aa ? payload_distance(v) : inf;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float t = __shfl_up(d, o);
                if (lane - o >= start) d = t < d ? t : d;
            }
            if (carried) d = c_min < d ? c_min : d;
            // their smallest distances one by one in lane order (= ascending model): every lane keeps the same sum
            for (unsigned long long cm = __ballot(closing && (m_cls & 1u)); cm; cm &= cm - 1ull)
                respersist_close_distance(r, __shfl(d, __ffsll((long long)cm) - 1));
            // ---- the step's last segment stays open
            open = true;
            c_f = __shfl(f, nv - 1);
            c_sf = __shfl(m_sf, nv - 1);
            c_cls = __shfl(m_cls, nv - 1);
            c_min = __shfl(d, nv - 1);
        }
        // the run ends: its last model closes (a run begins on a kept record, so there is one)
        if (open) {
            if (lane < TABLE_SIFT_BITS) r.cnt += (c_sf >> lane) & 1u;
            else if (lane < RESPERSIST_LANE_MODELS) r.cnt += (c_cls >> (lane - TABLE_SIFT_BITS)) & 1u;
            else if (lane == RESPERSIST_LANE_MODELS) r.cnt += 1u;
            if (c_cls & 1u) respersist_close_distance(r, c_min);
        }
        for (int o = 32; o > 0; o >>= 1) types |= __shfl_xor(types, o);
        if (lane < TABLE_SIFT_BITS) A.t_bits[row * TABLE_SIFT_BITS + lane] = (uint16_t)r.cnt;
        else if (lane < RESPERSIST_LANE_MODELS) A.t_cls[row * RESPERSIST_CLASSES + (lane - TABLE_SIFT_BITS)] = (uint16_t)r.cnt;
        else if (lane == RESPERSIST_LANE_MODELS) A.t_nmodels[row] = (uint16_t)r.cnt;
        else if (lane == RESPERSIST_LANE_CONTACTS) A.t_n[row] = r.cnt;
        if (lane == 0) {
            A.t_a[row] = (int)(k0 >> (A.rbits + A.fbits));
            A.t_b[row] = (int)((k0 >> A.fbits) & rmask);
            A.t_first[row] = (int)(k0 & fmask);
            A.t_last[row] = (int)c_f;
            A.t_dmin[row] = r.dmin;
            A.t_dmax[row] = r.dmax;
            A.t_dsum[row] = r.dsum;
            A.t_ctype[row] = (uint8_t)types;
        }
    }
}
