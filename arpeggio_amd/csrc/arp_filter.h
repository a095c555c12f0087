// arp_filter.h — the records of the atom-atom bag a caller asks for, picked on the device before the canonical sort
// (DESIGN.md 5h).  A record is kept when (sift & sift_any) != 0 and bit ctype of ctype_mask is set.  The filter reads the bag
// as the pass left it (out_i ... out_ct, in the order of the pair list) and writes the kept records, still in that order, into
// five columns of their own; arp_sort.h then sorts those alone.  Tiles of FILTER_TILE records, no atomics on global memory, no
// block waits for another:
//   k_filter_count  block t: kept records of tile t                                              -> tile_keep[t]
//   k_runs_scan     (arp_runs.h, one block) exclusive prefix of those counts over the tiles; their sum k' = kept records
//   (the host reads k' — the one wait — and sizes the filtered columns and their sorted slab)
//   k_filter_write  block t: the kept records of tile t at tile_keep[t] + rank in the tile, consecutive
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_runs.h"

#define FILTER_THREADS RUNS_THREADS
#define FILTER_ITEMS RUNS_ITEMS          // consecutive records per thread
#define FILTER_TILE (FILTER_THREADS * FILTER_ITEMS)
#define FILTER_CTYPES 7                  // ARP_CT_INTRA_NON_SELECTION ... ARP_CT_INTRA_BINDING_SITE

struct FilterArgs {
    // the bag of the pass, unsorted
    const int* ci;
    const int* cj;
    const float* d_in;
    const uint16_t* s_in;
    const uint8_t* ct_in;
    long long k;             // records
    uint32_t sift_any;       // low 15 bits
    uint32_t ctype_mask;     // low 7 bits
    int* tile_keep;          // [T]: kept records of tile t, then (k_runs_scan) their exclusive prefix
    // the kept records, in the order the bag holds them (k_filter_write)
    int* i_out;
    int* j_out;
    float* d_out;
    uint16_t* s_out;
    uint8_t* ct_out;
    long long kept;          // k'
};

// SIFt and contact type of the thread's FILTER_ITEMS consecutive records from lo on: one 16-byte and one 8-byte load where the
// eight are all there and the columns allow it, record by record otherwise (the last tile, a column that is a view at an odd
// offset).  Bit r of the result: record lo + r is kept.
__device__ __forceinline__ uint32_t filter_keep(const FilterArgs& A, long long lo, uint32_t sf[FILTER_ITEMS], uint32_t ct[FILTER_ITEMS]) {
    static_assert(FILTER_ITEMS == 8, "one uint4 of SIFt words and one uint2 of type bytes per thread");
    if (lo >= A.k) return 0u;
    const bool whole = lo + FILTER_ITEMS <= A.k && (((uintptr_t)(A.s_in + lo)) & 15) == 0 && (((uintptr_t)(A.ct_in + lo)) & 7) == 0;
    int n = FILTER_ITEMS;
    if (whole) {
        const uint4 s4 = *reinterpret_cast<const uint4*>(A.s_in + lo);
        const uint2 c2 = *reinterpret_cast<const uint2*>(A.ct_in + lo);
        const uint32_t sw[4] = {s4.x, s4.y, s4.z, s4.w};
        const uint32_t cw[2] = {c2.x, c2.y};
#pragma unroll
        for (int r = 0; r < FILTER_ITEMS; ++r) {
            sf[r] = (sw[r >> 1] >> (16 * (r & 1))) & 0xFFFFu;
            ct[r] = (cw[r >> 2] >> (8 * (r & 3))) & 0xFFu;
        }
    } else {
        n = (int)min((long long)FILTER_ITEMS, A.k - lo);
#pragma unroll
        for (int r = 0; r < FILTER_ITEMS; ++r) {
            sf[r] = r < n ? (uint32_t)A.s_in[lo + r] : 0u;
            ct[r] = r < n ? (uint32_t)A.ct_in[lo + r] : 0u;
        }
    }
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < FILTER_ITEMS; ++r) {
        const bool keep = r < n && (sf[r] & A.sift_any) != 0u && ct[r] < FILTER_CTYPES && ((A.ctype_mask >> ct[r]) & 1u) != 0u;
        m |= (keep ? 1u : 0u) << r;
    }
    return m;
}

__global__ __launch_bounds__(FILTER_THREADS) void k_filter_count(FilterArgs A) {
    __shared__ int s_w[FILTER_THREADS / 64];
    uint32_t sf[FILTER_ITEMS], ct[FILTER_ITEMS];
    int c = __popc(filter_keep(A, (long long)blockIdx.x * FILTER_TILE + (long long)threadIdx.x * FILTER_ITEMS, sf, ct));
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < FILTER_THREADS / 64; ++w) t += s_w[w];
        A.tile_keep[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(FILTER_THREADS) void k_filter_write(FilterArgs A) {
    __shared__ long long s_w[SORT_WAVES];
    static_assert(FILTER_THREADS == SORT_THREADS, "sort_block_scan scans SORT_THREADS values");
    const long long lo = (long long)blockIdx.x * FILTER_TILE + (long long)threadIdx.x * FILTER_ITEMS;
    uint32_t sf[FILTER_ITEMS], ct[FILTER_ITEMS];
    const uint32_t m = filter_keep(A, lo, sf, ct);
    long long pos = (long long)A.tile_keep[blockIdx.x] + sort_block_scan((long long)__popc(m), s_w, nullptr);
#pragma unroll
    for (int r = 0; r < FILTER_ITEMS; ++r)
        if ((m >> r) & 1u) {
            if (pos < A.kept) {      // (pos < k' always: k' is the sum of the same counts)
                A.i_out[pos] = A.ci[lo + r];
                A.j_out[pos] = A.cj[lo + r];
                A.d_out[pos] = A.d_in[lo + r];
                A.s_out[pos] = (uint16_t)sf[r];
                A.ct_out[pos] = (uint8_t)ct[r];
            }
            ++pos;
        }
}
