// arp_poses_clusters.h — leader clustering of the poses of the resident fingerprint result by fingerprint Tanimoto.
//
// The fingerprint result (arp_poses_fingerprints.h) is resident: bits [P][W] and count [P].  Nothing of it is written here: the
// kernels read it and write the clustering's own buffers.  Everything is an integer.
//
// The sequential definition — walk the positions, join the FIRST similar leader, else lead — runs in its round form:
//   k_pcl_round    round c, one launch.  next[c] is the leader's position (0xFFFFFFFF: no leader, the round returns at once).  A
//                  group of g lanes owns one position m: it leaves when m is assigned or in front of the leader; otherwise its
//                  lanes stride the W words of the pose's row and of the leader's row (staged in LDS when W <= PCL_LDS_WORDS,
//                  from L2 otherwise), one popcount of the AND a word, summed over the group by shuffles.  One lane computes q and
//                  either assigns m to c or proposes m for next[c + 1]: a minimum per thread over its positions, per wave by
//                  shuffles, per block through LDS, then ONE atomicMin a block behind a read that skips it when the stored
//                  value is lower already.  The leader's own group writes leader[c] and leader_position[c].  Round 0 meets every
//                  position and writes pose[m].
//   k_pcl_finish   one launch: C = the rounds whose next is not the sentinel, the unassigned count, and size — a histogram of
//                  cluster privatised per block in LDS (C <= 4096) before it touches global memory.
// No position is written by two groups and no group reads another position's cluster: a round has no race.  The rounds are
// ordered by the stream; no kernel waits for another block.  Every loop is bounded by W, M or max_clusters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PCL_MAX_CLUSTERS 4096        // ARP_POSECL_MAX_CLUSTERS
#define PCL_SENTINEL 0xFFFFFFFFu     // next[c]: no leader
#define PCL_LDS_WORDS 256            // the leader's row is staged in LDS up to this many words (2 KiB a block)
#define PCL_THREADS 256
#define PCL_ONE_Q32 (1ull << 32)

// words[4] of the launch's last wait
#define PCL_W_CLUSTERS 0
#define PCL_W_UNASSIGNED 1

struct PclArgs {
    // ---- the source
    const unsigned long long* bits;      // [P][W]; nullptr when W = 0 (never read then)
    const uint32_t* count;               // [P]
    long long W;
    // ---- the positions
    const int* order;                    // [M], or nullptr: position m names pose skip + m
    int skip, M;
    // ---- the rule
    unsigned long long threshold;        // q >= threshold: similar
    int max_clusters;
    int g, g_log2;                       // lanes per position: a power of two in [4, 64]
    // ---- the result
    uint32_t* next;                      // [max_clusters + 1]
    int* pose;                           // [M]
    int* cluster;                        // [M], -1 before a round assigns it
    long long* similarity;               // [M], -1 likewise
    int* leader;                         // [max_clusters]
    int* leader_position;                // [max_clusters]
    uint32_t* size;                      // [max_clusters], zeroed
    unsigned long long* words;           // [4], zeroed
};

// the power of two in [4, 64] at or above min(W, 64)
inline int pcl_group_width(long long W) {
    int g = 4;
    while (g < 64 && g < W) g <<= 1;
    return g;
}

__device__ __forceinline__ int pcl_pose_of(const PclArgs& A, int m) { return A.order ? A.order[m] : A.skip + m; }

// floor(t 2^32 / u), u = |a| + |b| - t; 0 / 0 is 1.0 (ARP_SHORTLIST_TANIMOTO's arithmetic; t < 2^32, so t << 32 fits)
__device__ __forceinline__ unsigned long long pcl_q32(uint32_t t, uint32_t a, uint32_t b) {
    const unsigned long long u = (unsigned long long)a + (unsigned long long)b - (unsigned long long)t;
    return u == 0ull ? PCL_ONE_Q32 : ((unsigned long long)t << 32) / u;
}

__global__ __launch_bounds__(PCL_THREADS) void k_pcl_round(PclArgs A, int c) {
    __shared__ unsigned long long s_row[PCL_LDS_WORDS];
    __shared__ uint32_t s_min[PCL_THREADS / 64];
    const uint32_t L = A.next[c];
    if (L == PCL_SENTINEL || L >= (uint32_t)A.M) return;      // (block-uniform; the second never: only positions are proposed)
    const int lp = pcl_pose_of(A, (int)L);
    const uint32_t lcount = A.count[lp];
    const long long W = A.W;
    const unsigned long long* lrow = A.bits + (long long)lp * W;      // (not dereferenced when W = 0)
    const bool staged = W <= PCL_LDS_WORDS;
    if (staged) {
        for (int w = (int)threadIdx.x; w < (int)W; w += PCL_THREADS) s_row[w] = lrow[w];
        __syncthreads();
    }
    const int g = A.g, gi = (int)threadIdx.x >> A.g_log2, li = (int)threadIdx.x & (g - 1);
    const int per_block = PCL_THREADS >> A.g_log2;
    uint32_t mine = PCL_SENTINEL;
    // (the loop's bounds are block-uniform: every lane of a wave reaches the shuffles)
    for (long long m0 = (long long)blockIdx.x * per_block; m0 < A.M; m0 += (long long)gridDim.x * per_block) {
        const long long m = m0 + gi;
        bool takes_part = m < A.M && m >= (long long)L;
        if (takes_part) takes_part = A.cluster[m] < 0;
        int p = 0;
        uint32_t t = 0;
        if (takes_part) {
            p = pcl_pose_of(A, (int)m);
            if (m != (long long)L) {
                const unsigned long long* const row = A.bits + (long long)p * W;
                if (staged)
                    for (long long w = li; w < W; w += g) t += (uint32_t)__popcll(row[w] & s_row[w]);
                else
                    for (long long w = li; w < W; w += g) t += (uint32_t)__popcll(row[w] & lrow[w]);
            }
        }
        for (int off = g >> 1; off > 0; off >>= 1) t += (uint32_t)__shfl_xor((int)t, off, 64);
        if (takes_part && li == 0) {
            if (c == 0) A.pose[m] = p;      // (round 0 meets every position)
            if (m == (long long)L) {
                A.cluster[m] = c;
                A.similarity[m] = (long long)PCL_ONE_Q32;
                A.leader[c] = p;
                A.leader_position[c] = (int)m;
            } else {
                const unsigned long long q = pcl_q32(t, A.count[p], lcount);
                if (q >= A.threshold) {
                    A.cluster[m] = c;
                    A.similarity[m] = (long long)q;
                } else if ((uint32_t)m < mine) mine = (uint32_t)m;
            }
        }
    }
    // ---- next[c + 1]: the lowest position that stays unassigned — per wave, per block, one atomic a block at the most
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mine, off, 64);
        mine = other < mine ? other : mine;
    }
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t lowest = s_min[0];
#pragma unroll
        for (int w = 1; w < PCL_THREADS / 64; ++w) lowest = s_min[w] < lowest ? s_min[w] : lowest;
        uint32_t* const slot = A.next + c + 1;
        if (lowest != PCL_SENTINEL && lowest < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, lowest);
    }
}

__global__ __launch_bounds__(PCL_THREADS) void k_pcl_finish(PclArgs A) {
    __shared__ uint32_t s_hist[PCL_MAX_CLUSTERS];
    __shared__ uint32_t s_unassigned, s_clusters;
    for (int b = (int)threadIdx.x; b < PCL_MAX_CLUSTERS; b += PCL_THREADS) s_hist[b] = 0u;
    if (threadIdx.x == 0) s_unassigned = s_clusters = 0u;
    __syncthreads();
    uint32_t unassigned = 0;
    for (long long m = (long long)blockIdx.x * PCL_THREADS + threadIdx.x; m < A.M; m += (long long)gridDim.x * PCL_THREADS) {
        const int cl = A.cluster[m];
        if (cl >= 0 && cl < A.max_clusters) atomicAdd(&s_hist[cl], 1u);
        else ++unassigned;
    }
    if (unassigned) atomicAdd(&s_unassigned, unassigned);
    if (blockIdx.x == 0) {
        uint32_t made = 0;
        for (int c = (int)threadIdx.x; c < A.max_clusters; c += PCL_THREADS) made += A.next[c] != PCL_SENTINEL ? 1u : 0u;
        if (made) atomicAdd(&s_clusters, made);
    }
    __syncthreads();
    for (int b = (int)threadIdx.x; b < A.max_clusters; b += PCL_THREADS)
        if (s_hist[b]) atomicAdd(&A.size[b], s_hist[b]);
    if (threadIdx.x == 0) {
        if (s_unassigned) atomicAdd(&A.words[PCL_W_UNASSIGNED], (unsigned long long)s_unassigned);
        if (blockIdx.x == 0) A.words[PCL_W_CLUSTERS] = (unsigned long long)s_clusters;
    }
}
