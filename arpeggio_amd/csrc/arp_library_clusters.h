// arp_library_clusters.h — leader clustering of the poses of the resident library fingerprint by fingerprint Tanimoto, in its
// window form.
//
// The library fingerprint (arp_library_fingerprints.h) is resident: bits [Q + T][W] and count [Q + T], the Q reference rows first.
// The launch hands the kernels the matrix FROM ROW Q ON, so pose t is row t here and a reference row is never met.  Nothing of the
// fingerprint, the library result or the library shortlist is written: the kernels read them and write the clustering's own
// buffers.  Everything is an integer; the similarity is pcl_q32 of arp_poses_clusters.h.
//
// The sequential definition — walk the positions, join the FIRST similar leader, else lead — runs in its window form, up to
// LCL_WINDOW leaders a round and two launches a round:
//   k_lcl_positions   a thread per position: pose[m] from the source (m itself, the uploaded list, or the shortlist's pose
//                     column, copied on the device) and ligand[m] = lig_of[pose[m]].  Every later kernel reads pose[], so the
//                     shortlist may be replaced behind the launch.
//   k_lcl_window(r)   ONE block.  start[r] is the lowest unassigned position (start[0] = 0; the sentinel: return at once); the
//                     window is [start, start + 32) within [0, M).  The block computes q for the pairs i < j of window positions
//                     that are both unassigned (a lane group strides the words of both rows — staged in LDS when 32 W <=
//                     LCL_LDS_WORDS, from L2 otherwise — and sums by shuffles), then wave 0 walks the window in order: lane k
//                     holds the k-th leader elected in this window, one ballot a candidate finds the first similar one.  A
//                     candidate with none leads while `made` < max_clusters and stays unassigned after that.  Writes cluster,
//                     similarity, leader, leader_position for the window, the round's leader positions wl[r][<= 32], their
//                     number nl[r], and `made`.  made == max_clusters on entry: nl[r] = 0 and nothing else.
//   k_lcl_sweep(r)    every unassigned position m >= start[r] + 32: a group of g lanes holds the words of m's row in registers
//                     (read once a round; beyond LCL_ROW_REGS words a lane they are read again from L1/L2), compares them with the
//                     nl[r] leader rows in leader order (staged in LDS when 32 W <= LCL_LDS_WORDS, from L2 otherwise), one
//                     shuffle reduction a leader, and joins the first similar one.  Otherwise m is a proposal for start[r + 1]:
//                     a minimum per thread, per wave by shuffles, per block through LDS, then ONE atomicMin a block behind a
//                     relaxed read that skips it when the stored value is lower already.  nl[r] = 0: return at once.  Once
//                     `made` has reached max_clusters nothing is proposed: the host reads the sentinel and stops.
//   k_lcl_finish      size as a histogram privatised in LDS, the unassigned count, C = made and the rounds that elected a leader.
//
// Why this is the sequential definition.  By induction over the rounds, a position that is unassigned when round r starts is
// similar to NO leader made before round r: the window positions of earlier rounds were compared with the leaders of their own
// window in order, and every position behind a window was swept against exactly that window's leaders.  start[r] is the first
// unassigned position, so the sequential walk makes it a leader too.  A window candidate j can, in the walk, only join a leader
// at a position < j; those made before the round are excluded by the induction, so only the leaders of its own window remain,
// and the wave meets them in leader order.  A position behind the window has met every earlier leader already, and the sweep
// compares it with the new ones in leader order: it joins the first similar leader overall.  Every round that runs elects at
// least start[r], and start advances by at least 32, so rounds <= min(max_clusters, ceil(M / 32)).
//
// No position is written by two groups in one kernel (the window kernel is one block and writes [start, start + 32); the sweep
// writes m >= start + 32, one group a position); no group reads another position's cluster.  The rounds are ordered by the
// stream: no cooperative launch, no kernel waits for another block.  Every loop is bounded by W, M, 32 or max_clusters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "arp_poses_clusters.h"      // pcl_q32, pcl_group_width, PCL_ONE_Q32, PCL_SENTINEL, PCL_MAX_CLUSTERS

#define LCL_WINDOW 32                // ARP_LIBCL_WINDOW: the positions a round resolves together
#define LCL_LDS_WORDS 2048           // ARP_LIBCL_LDS_WORDS: 32 rows are staged in LDS when 32 W <= this (16 KiB a block: W <= 64)
#define LCL_THREADS 256
#define LCL_ROW_REGS 4               // words of its own row a sweep lane keeps in registers (W <= 4 g: all of them)

// the source of the positions (ARP_LIBCL_*)
#define LCL_ALL 0
#define LCL_LIST 1
#define LCL_SHORTLIST 2

// words[4] of the launch's last wait
#define LCL_W_CLUSTERS 0
#define LCL_W_UNASSIGNED 1
#define LCL_W_ROUNDS 2

struct LclArgs {
    // ---- the source: the rows of the POSES (the launch has skipped the Q reference rows)
    const unsigned long long* bits;      // [T][W]; nullptr when W = 0 (never read then)
    const uint32_t* count;               // [T]
    long long W;
    const int* lig_of;                   // [T]
    const int* ids;                      // [M]: the uploaded list or the shortlist's pose column; nullptr: position m is pose m
    int M;
    // ---- the rule
    unsigned long long threshold;
    int max_clusters;
    int g, g_log2;                       // lanes per row pair / per position: a power of two in [4, 64]
    int rounds;                          // the rounds this launch can take: min(max_clusters, ceil(M / 32))
    // ---- the result
    uint32_t* start;                     // [rounds + 1]
    uint32_t* nl;                        // [rounds], zeroed
    int* wl;                             // [rounds][32]: the positions of the leaders elected in round r
    uint32_t* made;                      // [1], zeroed: the leaders so far
    int* pose;                           // [M]
    int* ligand;                         // [M]
    int* cluster;                        // [M], -1 before a round assigns it
    long long* similarity;               // [M], -1 likewise
    int* leader;                         // [max_clusters]
    int* leader_position;                // [max_clusters]
    uint32_t* size;                      // [max_clusters], zeroed
    unsigned long long* words;           // [4], zeroed
};

__global__ __launch_bounds__(LCL_THREADS) void k_lcl_positions(LclArgs A) {
    const long long m = (long long)blockIdx.x * LCL_THREADS + threadIdx.x;
    if (m >= A.M) return;
    const int p = A.ids ? A.ids[m] : (int)m;
    A.pose[m] = p;
    A.ligand[m] = A.lig_of[p];
}

__global__ __launch_bounds__(LCL_THREADS) void k_lcl_window(LclArgs A, int r) {
    __shared__ unsigned long long s_rows[LCL_LDS_WORDS];
    __shared__ unsigned long long s_q[LCL_WINDOW * LCL_WINDOW];      // [i][j], i < j
    __shared__ int s_pose[LCL_WINDOW];
    __shared__ uint32_t s_count[LCL_WINDOW];
    __shared__ int s_open[LCL_WINDOW];
    const uint32_t s = A.start[r];
    if (s == PCL_SENTINEL || s >= (uint32_t)A.M) return;      // (block-uniform)
    const uint32_t made0 = *A.made;
    if (made0 >= (uint32_t)A.max_clusters) {      // (the cap was reached in an earlier round: nothing is elected any more)
        if (threadIdx.x == 0) A.nl[r] = 0u;
        return;
    }
    const int n = min(LCL_WINDOW, A.M - (int)s);
    const long long W = A.W;
    if ((int)threadIdx.x < LCL_WINDOW) {
        const int i = (int)threadIdx.x;
        int p = 0, open = 0;
        if (i < n) { p = A.pose[s + i]; open = A.cluster[s + i] < 0 ? 1 : 0; }
        s_pose[i] = p;
        s_count[i] = i < n ? A.count[p] : 0u;
        s_open[i] = open;
    }
    __syncthreads();
    const bool staged = (long long)LCL_WINDOW * W <= LCL_LDS_WORDS;
    if (staged) {
        for (int e = (int)threadIdx.x; e < n * (int)W; e += LCL_THREADS) {
            const int i = e / (int)W, w = e - i * (int)W;
            s_rows[e] = A.bits[(long long)s_pose[i] * W + w];
        }
        __syncthreads();
    }
    // ---- q of the pairs i < j, both unassigned: a lane group a pair (the loop's bounds are block-uniform)
    // (at most 8 lanes a pair here: the one block has 32 x 32 table entries to visit, and 32 pairs a step instead of 4 at
    // W > 32 is what a round costs; the rows are in LDS or in L2, no HBM stream wants the wider group)
    const int g_log2 = min(A.g_log2, 3), g = 1 << g_log2, gi = (int)threadIdx.x >> g_log2, li = (int)threadIdx.x & (g - 1);
    const int per_block = LCL_THREADS >> g_log2;
    for (int e0 = 0; e0 < LCL_WINDOW * LCL_WINDOW; e0 += per_block) {
        const int e = e0 + gi, i = e >> 5, j = e & (LCL_WINDOW - 1);
        const bool takes_part = i < j && j < n && s_open[i] && s_open[j];
        uint32_t t = 0;
        if (takes_part) {
            if (staged) {
                const unsigned long long* const a = s_rows + (long long)i * W;
                const unsigned long long* const b = s_rows + (long long)j * W;
                for (long long w = li; w < W; w += g) t += (uint32_t)__popcll(a[w] & b[w]);
            } else {
                const unsigned long long* const a = A.bits + (long long)s_pose[i] * W;
                const unsigned long long* const b = A.bits + (long long)s_pose[j] * W;
                for (long long w = li; w < W; w += g) t += (uint32_t)__popcll(a[w] & b[w]);
            }
        }
        for (int off = g >> 1; off > 0; off >>= 1) t += (uint32_t)__shfl_xor((int)t, off, 64);
        if (takes_part && li == 0) s_q[e] = pcl_q32(t, s_count[i], s_count[j]);
    }
    __syncthreads();
    // ---- the walk: wave 0, lane k holds the k-th leader of this window (the loop and its branches are wave-uniform)
    if (threadIdx.x < 64) {
        const int lane = (int)threadIdx.x;
        int mine = 0, nlead = 0;
        uint32_t made = made0;
        for (int j = 0; j < n; ++j) {
            if (!s_open[j]) continue;
            const bool similar = lane < nlead && s_q[mine * LCL_WINDOW + j] >= A.threshold;      // (mine < j)
            const unsigned long long found = __ballot(similar);
            if (found) {
                const int k = __ffsll((long long)found) - 1;
                const int i = __shfl(mine, k, 64);
                if (lane == 0) {
                    A.cluster[s + j] = (int)made0 + k;
                    A.similarity[s + j] = (long long)s_q[i * LCL_WINDOW + j];
                }
            } else if (made < (uint32_t)A.max_clusters) {
                if (lane == nlead) mine = j;
                if (lane == 0) {
                    A.cluster[s + j] = (int)made;
                    A.similarity[s + j] = (long long)PCL_ONE_Q32;
                    A.leader[made] = s_pose[j];
                    A.leader_position[made] = (int)s + j;
                    A.wl[(long long)r * LCL_WINDOW + nlead] = (int)s + j;
                }
                ++nlead;
                ++made;
            }
        }
        if (lane == 0) {
            A.nl[r] = (uint32_t)nlead;
            *A.made = made;
        }
    }
}

__global__ __launch_bounds__(LCL_THREADS) void k_lcl_sweep(LclArgs A, int r) {
    __shared__ unsigned long long s_rows[LCL_LDS_WORDS];
    __shared__ int s_pose[LCL_WINDOW];
    __shared__ uint32_t s_count[LCL_WINDOW];
    __shared__ uint32_t s_min[LCL_THREADS / 64];
    const int nl = (int)A.nl[r];
    if (nl <= 0 || nl > LCL_WINDOW) return;      // (block-uniform; the second never)
    const long long first = (long long)A.start[r] + LCL_WINDOW;
    if (first >= A.M) return;                    // (nothing behind the window: start[r + 1] stays the sentinel)
    const uint32_t made = *A.made;               // (window r has run, window r + 1 has not)
    const int base = (int)made - nl;             // the cluster of this round's first leader
    const bool capped = made >= (uint32_t)A.max_clusters;      // no later round elects anyone: start[r + 1] stays the sentinel
    const long long W = A.W;
    if ((int)threadIdx.x < nl) {
        const int p = A.pose[A.wl[(long long)r * LCL_WINDOW + threadIdx.x]];
        s_pose[threadIdx.x] = p;
        s_count[threadIdx.x] = A.count[p];
    }
    __syncthreads();
    const bool staged = (long long)LCL_WINDOW * W <= LCL_LDS_WORDS;
    if (staged) {
        for (int e = (int)threadIdx.x; e < nl * (int)W; e += LCL_THREADS) {
            const int k = e / (int)W, w = e - k * (int)W;
            s_rows[e] = A.bits[(long long)s_pose[k] * W + w];
        }
        __syncthreads();
    }
    const int g = A.g, gi = (int)threadIdx.x >> A.g_log2, li = (int)threadIdx.x & (g - 1);
    const int per_block = LCL_THREADS >> A.g_log2;
    const bool in_regs = W <= (long long)LCL_ROW_REGS * g;
    uint32_t lowest = PCL_SENTINEL;
    // (the loops' bounds are block-uniform: every lane of a wave reaches the shuffles)
    for (long long m0 = first + (long long)blockIdx.x * per_block; m0 < A.M; m0 += (long long)gridDim.x * per_block) {
        const long long m = m0 + gi;
        bool takes_part = m < A.M;
        if (takes_part) takes_part = A.cluster[m] < 0;
        int p = 0;
        uint32_t pcount = 0;
        unsigned long long own[LCL_ROW_REGS] = {0ull, 0ull, 0ull, 0ull};
        const unsigned long long* row = A.bits;
        if (takes_part) {
            p = A.pose[m];
            pcount = A.count[p];
            row = A.bits + (long long)p * W;
            if (in_regs) {
#pragma unroll
                for (int x = 0; x < LCL_ROW_REGS; ++x) {
                    const long long w = li + (long long)x * g;
                    if (w < W) own[x] = row[w];
                }
            }
        }
        int joined = -1;
        unsigned long long joined_q = 0ull;
        for (int k = 0; k < nl; ++k) {
            uint32_t t = 0;
            if (takes_part && joined < 0) {
                const unsigned long long* const lrow = staged ? s_rows + (long long)k * W : A.bits + (long long)s_pose[k] * W;
                if (in_regs) {
#pragma unroll
                    for (int x = 0; x < LCL_ROW_REGS; ++x) {
                        const long long w = li + (long long)x * g;
                        if (w < W) t += (uint32_t)__popcll(own[x] & lrow[w]);
                    }
                } else {
                    for (long long w = li; w < W; w += g) t += (uint32_t)__popcll(row[w] & lrow[w]);
                }
            }
            for (int off = g >> 1; off > 0; off >>= 1) t += (uint32_t)__shfl_xor((int)t, off, 64);
            if (takes_part && joined < 0) {      // (every lane of the group holds the same t)
                const unsigned long long q = pcl_q32(t, pcount, s_count[k]);
                if (q >= A.threshold) { joined = k; joined_q = q; }
            }
        }
        if (takes_part && li == 0) {
            if (joined >= 0) {
                A.cluster[m] = base + joined;
                A.similarity[m] = (long long)joined_q;
            } else if ((uint32_t)m < lowest) lowest = (uint32_t)m;
        }
    }
    // ---- start[r + 1]: the lowest position that stays unassigned — per wave, per block, one atomic a block at the most
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)lowest, off, 64);
        lowest = other < lowest ? other : lowest;
    }
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = lowest;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t low = s_min[0];
#pragma unroll
        for (int w = 1; w < LCL_THREADS / 64; ++w) low = s_min[w] < low ? s_min[w] : low;
        uint32_t* const slot = A.start + r + 1;
        if (!capped && low != PCL_SENTINEL && low < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, low);
    }
}

__global__ __launch_bounds__(LCL_THREADS) void k_lcl_finish(LclArgs A) {
    __shared__ uint32_t s_hist[PCL_MAX_CLUSTERS];
    __shared__ uint32_t s_unassigned, s_rounds;
    for (int b = (int)threadIdx.x; b < PCL_MAX_CLUSTERS; b += LCL_THREADS) s_hist[b] = 0u;
    if (threadIdx.x == 0) s_unassigned = s_rounds = 0u;
    __syncthreads();
    uint32_t unassigned = 0;
    for (long long m = (long long)blockIdx.x * LCL_THREADS + threadIdx.x; m < A.M; m += (long long)gridDim.x * LCL_THREADS) {
        const int cl = A.cluster[m];
        if (cl >= 0 && cl < A.max_clusters) atomicAdd(&s_hist[cl], 1u);
        else ++unassigned;
    }
    if (unassigned) atomicAdd(&s_unassigned, unassigned);
    if (blockIdx.x == 0) {
        uint32_t ran = 0;
        for (int q = (int)threadIdx.x; q < A.rounds; q += LCL_THREADS) ran += A.nl[q] != 0u ? 1u : 0u;
        if (ran) atomicAdd(&s_rounds, ran);
    }
    __syncthreads();
    for (int b = (int)threadIdx.x; b < A.max_clusters; b += LCL_THREADS)
        if (s_hist[b]) atomicAdd(&A.size[b], s_hist[b]);
    if (threadIdx.x == 0) {
        if (s_unassigned) atomicAdd(&A.words[LCL_W_UNASSIGNED], (unsigned long long)s_unassigned);
        if (blockIdx.x == 0) {
            A.words[LCL_W_CLUSTERS] = (unsigned long long)*A.made;
            A.words[LCL_W_ROUNDS] = (unsigned long long)s_rounds;
        }
    }
}
