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
//   k_residue_rekey         atom-atom record p -> key respersist_key (here, fbits = 0: res_a << rbits | res_b), payload
//                           table_payload (arp_runs.h), class 0
//   k_residue_rekey_planes  the records of the four ring / amide bags behind them, class 1 ... 4, no distance / SIFt / type
//   (radix passes of arp_sort.h over every bit of the key: k_sort_hist / k_sort_scan / k_sort_scatter, up to 9 bits a pass)
//   k_runs_count / k_runs_scan / k_runs_starts (arp_runs.h, shift 0): the runs of equal keys; U = rows
//   k_respair_reduce        one wave per row, 64 records of the run per step
// The two re-key kernels are also those of the residue persistence table (arp_respersist.h), whose key carries the model
// in its low fbits bits; this table passes fbits = 0 and nres_t = every resident residue, so that f is 0 for every id.
//
// Records that are LEFT OUT (a ring or amide without a residue: -1) keep their slot: their key is all ones and their class
// TABLE_LEFT_OUT.  All ones sorts behind every pair (see respersist_key_bits), k_runs_count never lets such a record begin a
// run, so they trail the last run and k_respair_reduce, which counts by class, passes over them.  The alternative — compacting
// them away with ballot-ranked writes — would tell the host how many records the sort has only after a second wait.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_runs.h"

#define RESPAIR_PLANE_BAGS 4     // atom-plane, plane-plane, group-group, group-plane: classes 1 ... 4

// one ring / amide bag: its two id columns, the residue tables they index, its records and where they go
struct RespairBag {
    const int* a;
    const int* b;
    const int* res_of_a;
    const int* res_of_b;
    long long count;
    long long out;           // first slot of the bag's records in key / val
};

// what re-keying the five bags of a pass by residue reads and writes (both residue tables)
struct RekeyArgs {
    // the atom-atom bag of the last pass, in the order the pass left it
    const int* ci;
    const int* cj;
    const float* d_in;
    const uint16_t* s_in;
    const uint8_t* ct_in;
    const int* res_id;
    long long k_aa;          // its records
    RespairBag bag[RESPAIR_PLANE_BAGS];
    uint32_t nres_t;         // residues of the topology (resident residues of model f: [f nres_t, (f + 1) nres_t)); >= 1
    int rbits, fbits;        // key = res_a << (rbits + fbits) | res_b << fbits | f
    unsigned long long* key;
    unsigned long long* val;
};

struct RespairArgs {
    int rbits;               // key = res_a << rbits | res_b
    // the re-keyed records, sorted
    const unsigned long long* key;
    const unsigned long long* val;
    const int* row_start;    // [U + 1] (RunArgs)
    long long U;
    // the table, one column after the other (RESPAIR_TABLE)
    int* t_a;
    int* t_b;
    uint32_t* t_n;
    float* t_dmin;
    uint32_t* t_bits;        // [U][TABLE_SIFT_BITS]
    uint8_t* t_ctype;
    uint32_t* t_planes;      // [U][RESPAIR_PLANE_BAGS]
};

// the unordered topology pair and the model as a key; a negative residue leaves the record out.  Both residues lie in the
// same model, so the model of either is the record's.
__device__ __forceinline__ bool respersist_key(int ra, int rb, const RekeyArgs& A, unsigned long long* key) {
    if ((ra | rb) < 0) { *key = ~0ull; return false; }
    const uint32_t f = (uint32_t)ra / A.nres_t;
    const uint32_t base = f * A.nres_t;
    const uint32_t lo = (uint32_t)min(ra, rb) - base, hi = (uint32_t)max(ra, rb) - base;
    *key = ((unsigned long long)lo << (A.rbits + A.fbits)) | ((unsigned long long)hi << A.fbits) | (unsigned long long)f;
    return true;
}

__global__ __launch_bounds__(256) void k_residue_rekey(RekeyArgs A) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < A.k_aa; p += (long long)gridDim.x * blockDim.x) {
        unsigned long long key;
        const bool kept = respersist_key(A.res_id[A.ci[p]], A.res_id[A.cj[p]], A, &key);
        A.key[p] = key;
        A.val[p] = kept ? table_payload(A.d_in[p], A.s_in[p], A.ct_in[p], 0ull) : TABLE_LEFT_OUT << TABLE_CLASS_SHIFT;
    }
}

// grid (x, RESPAIR_PLANE_BAGS): row y of the grid walks bag y
__global__ __launch_bounds__(256) void k_residue_rekey_planes(RekeyArgs A) {
    const RespairBag g = A.bag[blockIdx.y];
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < g.count; p += (long long)gridDim.x * blockDim.x) {
        unsigned long long key;
        const bool kept = respersist_key(g.res_of_a[g.a[p]], g.res_of_b[g.b[p]], A, &key);
        A.key[g.out + p] = key;
        A.val[g.out + p] = (kept ? (unsigned long long)(blockIdx.y + 1) : TABLE_LEFT_OUT) << TABLE_CLASS_SHIFT;
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
            const unsigned long long v = q + lane < e ? A.val[q + lane] : TABLE_LEFT_OUT << TABLE_CLASS_SHIFT;
            const uint32_t cls = payload_class(v);
            const bool aa = cls == 0u;
            const uint32_t sf = payload_sift(v);
            if (aa) {
                const float d = payload_distance(v);
                dmin = d < dmin ? d : dmin;
                types |= 1u << payload_type(v);
            }
#pragma unroll
            for (int b = 0; b < TABLE_SIFT_BITS; ++b) {
                const uint32_t c = (uint32_t)__popcll(__ballot(aa && ((sf >> b) & 1u)));
                if (lane == b) cnt += c;
            }
#pragma unroll
            for (int m = 0; m <= RESPAIR_PLANE_BAGS; ++m) {
                const uint32_t c = (uint32_t)__popcll(__ballot(cls == (uint32_t)m));
                if (lane == TABLE_SIFT_BITS + m) cnt += c;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float omin = __shfl_xor(dmin, o);
            dmin = omin < dmin ? omin : dmin;
            types |= __shfl_xor(types, o);
        }
        if (lane < TABLE_SIFT_BITS) A.t_bits[row * TABLE_SIFT_BITS + lane] = cnt;
        else if (lane == TABLE_SIFT_BITS) A.t_n[row] = cnt;
        else if (lane <= TABLE_SIFT_BITS + RESPAIR_PLANE_BAGS) A.t_planes[row * RESPAIR_PLANE_BAGS + (lane - TABLE_SIFT_BITS - 1)] = cnt;
        if (lane == 0) {
            A.t_a[row] = (int)(k0 >> A.rbits);
            A.t_b[row] = (int)(k0 & rmask);
            A.t_dmin[row] = dmin;
            A.t_ctype[row] = (uint8_t)types;
        }
    }
}
