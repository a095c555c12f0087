// arp_persist.h — contact persistence over the models of an ensemble, reduced on the device.
//
// After a pass over F resident models (arp_set_models) the atom-atom bag holds, for every model f, the records of that model
// with ids f n + a.  What a user of an ensemble wants is one row per topology pair (a, b): in how many models the contact
// exists, how often each SIFt bit is set, the range and the sum of the distances.  The rows are a regrouping of records
// that are already resident, so they are made here and only the table crosses PCIe.
//
// Shape: the bag is re-keyed to (a, b, f) and sorted by the WHOLE key with the radix passes of arp_sort.h (k_sort_hist /
// k_sort_scan / k_sort_scatter; least significant digit first, stable, no atomics on global memory).  k_sort_runs is not
// used: it ranks the records of a run by their second id and needs those to be distinct, which (a, b) over F models are
// not.  Sorting every bit of the key needs no tie-break and no per-atom stage in LDS: an atom with 10^4 records (they
// grow with F) is sorted like any other, so there is no capacity and no second path (ARP_PERSIST_STAGE_MAX = 0).
// After the sort the records of a pair are one run in ascending f:
//   k_persist_rekey   record p -> key a << (bbits + fbits) | b << fbits | f, payload table_payload (arp_runs.h), class 0
//   (radix passes over the abits + bbits + fbits bits of the key, up to 9 bits a pass)
//   k_runs_count / k_runs_scan / k_runs_starts (arp_runs.h, shift fbits): a run = a record whose (a, b) differs from its
//   predecessor's; the host reads their number U — the one wait — and sizes the table
//   k_persist_reduce  one wave per row: 64 records of the run per step, consecutive lanes on consecutive records;
//                     counts by ballots, min / max / type mask by a butterfly over the lanes, and dist_sum by adding the 64
//                     distances of a step ONE BY ONE in lane order (= ascending model) to the running float64 sum — the
//                     order the table's contract fixes.  No tree reduction touches dist_sum.
// The sort's input is the bag as the pass left it (the unsorted columns), so nothing here reads or writes the sorted slab:
// the canonical order of the bag, its layout (records / rows) and arp_set_sort_after_pass neither change the table nor are
// changed by it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_runs.h"

struct PersistArgs {
    // the bag of the last pass, in the order the pass left it
    const int* ci;
    const int* cj;
    const float* d_in;
    const uint16_t* s_in;
    const uint8_t* ct_in;
    long long k;             // records
    uint32_t n;              // atoms of the topology (ids of model f: [f n, (f + 1) n))
    int bbits, fbits;        // key = a << (bbits + fbits) | b << fbits | f
    // re-keyed records: written by k_persist_rekey, read (sorted) by everything after the radix passes
    unsigned long long* key;
    unsigned long long* val;
    const int* row_start;    // [U + 1]: first record of row r; row_start[U] = k (RunArgs)
    long long U;
    // the table, one column after the other (PERSIST_TABLE)
    int* t_a;
    int* t_b;
    uint16_t* t_nmodels;
    int* t_first;
    int* t_last;
    float* t_dmin;
    float* t_dmax;
    double* t_dsum;
    uint16_t* t_bits;        // [U][TABLE_SIFT_BITS]
    uint8_t* t_ctype;
};

__global__ __launch_bounds__(256) void k_persist_rekey(PersistArgs A) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < A.k; p += (long long)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)A.ci[p], j = (uint32_t)A.cj[p];
        const uint32_t f = i / A.n;                  // (a pair never crosses models: j lies in the same model)
        const uint32_t base = f * A.n;
        A.key[p] = ((unsigned long long)(i - base) << (A.bbits + A.fbits)) | ((unsigned long long)(j - base) << A.fbits) | (unsigned long long)f;
        A.val[p] = table_payload(A.d_in[p], A.s_in[p], A.ct_in[p], 0ull);
    }
}

__global__ __launch_bounds__(256) void k_persist_reduce(PersistArgs A) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const unsigned long long fmask = (1ull << A.fbits) - 1ull, bmask = (1ull << A.bbits) - 1ull;
    for (long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < A.U; row += waves) {
        const long long s = A.row_start[row], e = A.row_start[row + 1];
        const unsigned long long k0 = A.key[s], k1 = A.key[e - 1];
        float dmin = 0.f, dmax = 0.f;
        bool seen = false;
        uint32_t types = 0;
        int cnt = 0;              // lane b < TABLE_SIFT_BITS: records of the run with SIFt bit b
        double sum = 0.0;
        for (long long q = s; q < e; q += 64) {      // (wave-uniform trip count)
            const bool valid = q + lane < e;
            const unsigned long long v = valid ? A.val[q + lane] : 0ull;
            const float d = payload_distance(v);
            const uint32_t sf = payload_sift(v);
            if (valid) {
                dmin = seen ? (d < dmin ? d : dmin) : d;
                dmax = seen ? (d > dmax ? d : dmax) : d;
                seen = true;
                types |= 1u << payload_type(v);
            }
#pragma unroll
            for (int b = 0; b < TABLE_SIFT_BITS; ++b) {
                const int c = __popcll(__ballot(valid && ((sf >> b) & 1u)));
                if (lane == b) cnt += c;
            }
            // the distances of this step in ascending model order, one by one (every lane keeps the same sum)
            const int m = (int)(e - q < 64 ? e - q : 64);
            for (int l = 0; l < m; ++l) sum += (double)__shfl(d, l);
        }
        // lanes without a record (a run shorter than 64) take a neighbour's value as soon as they meet one
        for (int o = 32; o > 0; o >>= 1) {
            const float omin = __shfl_xor(dmin, o), omax = __shfl_xor(dmax, o);
            const int oseen = __shfl_xor(seen ? 1 : 0, o);
            types |= __shfl_xor(types, o);
            if (oseen) {
                dmin = seen ? (omin < dmin ? omin : dmin) : omin;
                dmax = seen ? (omax > dmax ? omax : dmax) : omax;
                seen = true;
            }
        }
        if (lane < TABLE_SIFT_BITS) A.t_bits[row * TABLE_SIFT_BITS + lane] = (uint16_t)cnt;
        if (lane == 0) {
            A.t_a[row] = (int)(k0 >> (A.bbits + A.fbits));
            A.t_b[row] = (int)((k0 >> A.fbits) & bmask);
            A.t_nmodels[row] = (uint16_t)(e - s);
            A.t_first[row] = (int)(k0 & fmask);
            A.t_last[row] = (int)(k1 & fmask);
            A.t_dmin[row] = dmin;
            A.t_dmax[row] = dmax;
            A.t_dsum[row] = sum;
            A.t_ctype[row] = (uint8_t)types;
        }
    }
}
