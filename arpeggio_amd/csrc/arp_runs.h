// arp_runs.h — the runs of a sorted key array, found on the device, and the payload the device-reduced tables sort beside
// their keys.  Nothing here belongs to one table: arp_persist.h, arp_respair.h and arp_respersist.h all find
// their rows with these kernels and pack their records with table_payload; arp_bridge.h and arp_bridgepersist.h find their
// runs with them too.
//   k_runs_count   block t: the runs that BEGIN in tile t (a record whose key >> shift differs from its predecessor's)
//   k_runs_scan    one block: exclusive prefix of those counts over the tiles; their sum U = rows of the table
//   (the host reads U — the one wait — and sizes the table)
//   k_runs_starts  block t: row_start[prefix[t] + rank in the tile] = position of the run's first record
//   scan_round     a round of 1024 values of a prefix sum with a running carry: the offsets kernels of the pose results
//                  (arp_poses.h, arp_poses_shortlist.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_sort.h"

#define RUNS_THREADS 256
#define RUNS_ITEMS 8             // consecutive records per thread of k_runs_count / k_runs_starts
#define RUNS_TILE (RUNS_THREADS * RUNS_ITEMS)

#define TABLE_SIFT_BITS 15       // SIFt bits with a column of their own (ARP_S_CLASH ... ARP_S_WEAK_POLAR)
#define TABLE_TYPE_SHIFT 47
#define TABLE_CLASS_SHIFT 50
#define TABLE_LEFT_OUT 7ull      // class of a record without a row (a residue of -1)

// The 64-bit payload of a record: distance | (SIFt & 0x7FFF) << 32 | (type & 7) << 47 | class << 50.  Class 0 is an atom-atom
// record; the residue tables give the ring / amide bags classes 1 ... 4 (no distance / SIFt / type) and TABLE_LEFT_OUT.
__device__ __forceinline__ unsigned long long table_payload(float d, uint32_t sift, uint32_t type, unsigned long long cls) {
    return (unsigned long long)__float_as_uint(d) | ((unsigned long long)(sift & 0x7FFFu) << 32) |
           ((unsigned long long)(type & 7u) << TABLE_TYPE_SHIFT) | (cls << TABLE_CLASS_SHIFT);
}
__device__ __forceinline__ float payload_distance(unsigned long long v) { return __uint_as_float((uint32_t)v); }
__device__ __forceinline__ uint32_t payload_sift(unsigned long long v) { return (uint32_t)(v >> 32) & 0x7FFFu; }
__device__ __forceinline__ uint32_t payload_type(unsigned long long v) { return (uint32_t)(v >> TABLE_TYPE_SHIFT) & 7u; }
__device__ __forceinline__ uint32_t payload_class(unsigned long long v) { return (uint32_t)(v >> TABLE_CLASS_SHIFT) & 7u; }

// One round of a block-wide prefix sum over more values than the block has threads: the 1024 threads (16 waves) of a block each
// bring one value of the round, get the sum of everything before it — the rounds before included, through `carry`, which every
// thread keeps and which ends as the sum of all rounds — and go on to the next round.  Every thread of the block calls it, the
// same number of times.  s_w is the caller's: 16 words of shared memory that nothing else uses between the rounds.
__device__ __forceinline__ unsigned long long scan_round(unsigned long long v, unsigned long long* s_w, unsigned long long& carry) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long u = __shfl_up(incl, d);
        if (lane >= d) incl += u;
    }
    __syncthreads();      // (s_w: read in the round before)
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    unsigned long long before = carry;
    for (int k = 0; k < wv; ++k) before += s_w[k];
    for (int k = 0; k < 16; ++k) carry += s_w[k];
    return before + incl - v;
}

// What finding the runs of a sorted key array needs: a run = consecutive records with equal key >> shift.  A record whose
// key >> shift is all ones (~0ull >> shift) never BEGINS a run: no key of the persistence table has 64 bits, and the
// residue tables mark the records they leave out that way (they sort last and trail the last run uncounted).
struct RunArgs {
    const unsigned long long* key;   // sorted
    long long k;             // records
    int shift;
    int T;                   // tiles of RUNS_TILE records
    int* tile_rows;          // [T]: runs beginning in tile t, then their exclusive prefix
    long long* total;        // [1]: U
    int* row_start;          // [U + 1]: first record of row r; row_start[U] = k
    long long U;
};

// bit r of the result: record lo + r of the thread's RUNS_ITEMS consecutive records begins a run
__device__ __forceinline__ uint32_t run_heads(const RunArgs& A, long long lo) {
    if (lo >= A.k) return 0u;
    const unsigned long long none = ~0ull >> A.shift;
    unsigned long long prev = lo > 0 ? (A.key[lo - 1] >> A.shift) : none;
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < RUNS_ITEMS; ++r) {
        if (lo + r >= A.k) break;
        const unsigned long long cur = A.key[lo + r] >> A.shift;
        m |= (cur != prev && cur != none ? 1u : 0u) << r;
        prev = cur;
    }
    return m;
}

__global__ __launch_bounds__(RUNS_THREADS) void k_runs_count(RunArgs A) {
    __shared__ int s_w[RUNS_THREADS / 64];
    int c = __popc(run_heads(A, (long long)blockIdx.x * RUNS_TILE + (long long)threadIdx.x * RUNS_ITEMS));
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < RUNS_THREADS / 64; ++w) t += s_w[w];
        A.tile_rows[blockIdx.x] = t;
    }
}

// one block (SORT_THREADS threads: sort_block_scan)
__global__ __launch_bounds__(SORT_THREADS) void k_runs_scan(RunArgs A) {
    __shared__ long long s_w[SORT_WAVES];
    long long run = 0;
    for (int t0 = 0; t0 < A.T; t0 += SORT_THREADS) {      // (block-uniform trip count)
        const int t = t0 + threadIdx.x;
        const int v = t < A.T ? A.tile_rows[t] : 0;
        long long sum;
        const long long e = sort_block_scan((long long)v, s_w, &sum);
        if (t < A.T) A.tile_rows[t] = (int)(run + e);      // (rows <= records < 2^31)
        run += sum;
    }
    if (threadIdx.x == 0) A.total[0] = run;
}

__global__ __launch_bounds__(RUNS_THREADS) void k_runs_starts(RunArgs A) {
    __shared__ long long s_w[SORT_WAVES];
    static_assert(RUNS_THREADS == SORT_THREADS, "sort_block_scan scans SORT_THREADS values");
    const long long lo = (long long)blockIdx.x * RUNS_TILE + (long long)threadIdx.x * RUNS_ITEMS;
    const uint32_t m = run_heads(A, lo);
    long long row = (long long)A.tile_rows[blockIdx.x] + sort_block_scan((long long)__popc(m), s_w, nullptr);
#pragma unroll
    for (int r = 0; r < RUNS_ITEMS; ++r)
        if ((m >> r) & 1u) {
            if (row < A.U) A.row_start[row] = (int)(lo + r);      // (row < U always: U is the sum of the same counts)
            ++row;
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) A.row_start[A.U] = (int)A.k;
}
