// arp_respair.h — the residue-residue contact table of a pass, reduced on the device.
//
// Every bag of a pass is per atom pair or per ring / amide pair; the first thing a consumer does is fold the records by
// residue.  The fold is a regrouping of records that are resident after the pass, and the table is much smaller than they
// are, so it is made here and only the table crosses PCIe: one row per unordered residue pair (res_a <= res_b) with at least
// one record in any of the five bags — atom-atom records counted with their SIFt bits, their smallest distance and their
// contact types, the records of the four ring / amide bags counted per bag.  Every column is a count, a minimum or an OR:
// the table is a function of the bags as SETS of records, whatever order the pass wrote them in.
//
// Shape (that of the persistence table, arp_persist.h):
//   k_respair_rekey         atom-atom record p -> key res_a << rbits | res_b, payload distance | SIFt << 32 | type << 47, class 0
//   k_respair_rekey_planes  the records of the four ring / amide bags behind them, class 1 ... 4, no distance / SIFt / type
//   (radix passes of arp_sort.h over every bit of the key: k_sort_hist / k_sort_scan / k_sort_scatter, up to 9 bits a pass)
//   k_persist_count / k_persist_scan / k_persist_starts (arp_persist.h, shift 0): the runs of equal keys; U = rows
//   k_respair_reduce        one wave per row, 64 records of the run per step
//
// Records that are LEFT OUT (a ring or amide without a residue: -1) keep their slot: their key is all ones and their class
// RESPAIR_LEFT_OUT.  All ones sorts behind every pair (see respair_key_bits), k_persist_count never lets such a record begin a
// run, so they trail the last run and k_respair_reduce, which counts by class, passes over them.  The alternative — compacting
// them away with ballot-ranked writes — would tell the host how many records the sort has only after a second wait.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_persist.h"

#define RESPAIR_BITS 15          // SIFt bits with a column of their own (ARP_S_CLASH ... ARP_S_WEAK_POLAR)
#define RESPAIR_PLANE_BAGS 4     // atom-plane, plane-plane, group-group, group-plane: classes 1 ... 4
#define RESPAIR_LEFT_OUT 7ull    // class of a record without a residue pair
#define RESPAIR_CLASS_SHIFT 50

// one ring / amide bag: its two id columns, the residue tables they index, its records and where they go
struct RespairBag {
    const int* a;
    const int* b;
    const int* res_of_a;
    const int* res_of_b;
    long long count;
    long long out;           // first slot of the bag's records in key / val
};

struct RespairArgs {
    // the atom-atom bag of the last pass, in the order the pass left it
    const int* ci;
    const int* cj;
    const float* d_in;
    const uint16_t* s_in;
    const uint8_t* ct_in;
    const int* res_id;
    long long k_aa;          // its records
    RespairBag bag[RESPAIR_PLANE_BAGS];
    int rbits;               // key = res_a << rbits | res_b
    // re-keyed records: written by the two rekey kernels, read (sorted) by everything after the radix passes
    unsigned long long* key;
    unsigned long long* val;
    const int* row_start;    // [U + 1] (RunArgs)
    long long U;
    // the table, one column after the other (respair_layout)
    int* t_a;
    int* t_b;
    uint32_t* t_n;
    float* t_dmin;
    uint32_t* t_bits;        // [U][RESPAIR_BITS]
    uint8_t* t_ctype;
    uint32_t* t_planes;      // [U][RESPAIR_PLANE_BAGS]
};

// the unordered pair as a key; a negative residue leaves the record out
__device__ __forceinline__ bool respair_key(int ra, int rb, int rbits, unsigned long long* key) {
    if ((ra | rb) < 0) { *key = ~0ull; return false; }
    const uint32_t lo = (uint32_t)min(ra, rb), hi = (uint32_t)max(ra, rb);
    *key = ((unsigned long long)lo << rbits) | (unsigned long long)hi;
    return true;
}

__global__ __launch_bounds__(256) void k_respair_rekey(RespairArgs A) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < A.k_aa; p += (long long)gridDim.x * blockDim.x) {
        unsigned long long key;
        const bool kept = respair_key(A.res_id[A.ci[p]], A.res_id[A.cj[p]], A.rbits, &key);
        A.key[p] = key;
        A.val[p] = kept ? (unsigned long long)__float_as_uint(A.d_in[p]) | ((unsigned long long)(A.s_in[p] & 0x7FFFu) << 32) |
                              ((unsigned long long)(A.ct_in[p] & 7u) << 47)
                        : RESPAIR_LEFT_OUT << RESPAIR_CLASS_SHIFT;
    }
}

// grid (x, RESPAIR_PLANE_BAGS): row y of the grid walks bag y
__global__ __launch_bounds__(256) void k_respair_rekey_planes(RespairArgs A) {
    const RespairBag g = A.bag[blockIdx.y];
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < g.count; p += (long long)gridDim.x * blockDim.x) {
        unsigned long long key;
        const bool kept = respair_key(g.res_of_a[g.a[p]], g.res_of_b[g.b[p]], A.rbits, &key);
        A.key[g.out + p] = key;
        A.val[g.out + p] = (kept ? (unsigned long long)(blockIdx.y + 1) : RESPAIR_LEFT_OUT) << RESPAIR_CLASS_SHIFT;
    }
}

__global__ __launch_bounds__(256) void k_respair_reduce(RespairArgs A) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const unsigned long long rmask = (1ull << A.rbits) - 1ull;
    for (long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < A.U; row += waves) {
        // (the last row's range also holds the left-out records that trail it: their class counts nowhere)
        const long long s = A.row_start[row], e = A.row_start[row + 1];
        const unsigned long long k0 = A.key[s];
        float dmin = __uint_as_float(0x7F800000u);      // +inf: no atom-atom record met
        uint32_t types = 0;
        uint32_t cnt = 0;         // lane b < 15: atom-atom records with SIFt bit b; lane 15: atom-atom records; lane 15 + m: records of class m
        for (long long q = s; q < e; q += 64) {      // (wave-uniform trip count)
            const unsigned long long v = q + lane < e ? A.val[q + lane] : RESPAIR_LEFT_OUT << RESPAIR_CLASS_SHIFT;
            const uint32_t cls = (uint32_t)(v >> RESPAIR_CLASS_SHIFT) & 7u;
            const bool aa = cls == 0u;
            const uint32_t sf = (uint32_t)(v >> 32) & 0x7FFFu;
            if (aa) {
                const float d = __uint_as_float((uint32_t)v);
                dmin = d < dmin ? d : dmin;
                types |= 1u << ((uint32_t)(v >> 47) & 7u);
            }
#pragma unroll
            for (int b = 0; b < RESPAIR_BITS; ++b) {
                const uint32_t c = (uint32_t)__popcll(__ballot(aa && ((sf >> b) & 1u)));
                if (lane == b) cnt += c;
            }
#pragma unroll
            for (int m = 0; m <= RESPAIR_PLANE_BAGS; ++m) {
                const uint32_t c = (uint32_t)__popcll(__ballot(cls == (uint32_t)m));
                if (lane == RESPAIR_BITS + m) cnt += c;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float omin = __shfl_xor(dmin, o);
            dmin = omin < dmin ? omin : dmin;
            types |= __shfl_xor(types, o);
        }
        if (lane < RESPAIR_BITS) A.t_bits[row * RESPAIR_BITS + lane] = cnt;
        else if (lane == RESPAIR_BITS) A.t_n[row] = cnt;
        else if (lane <= RESPAIR_BITS + RESPAIR_PLANE_BAGS) A.t_planes[row * RESPAIR_PLANE_BAGS + (lane - RESPAIR_BITS - 1)] = cnt;
        if (lane == 0) {
            A.t_a[row] = (int)(k0 >> A.rbits);
            A.t_b[row] = (int)(k0 & rmask);
            A.t_dmin[row] = dmin;
            A.t_ctype[row] = (uint8_t)types;
        }
    }
}
