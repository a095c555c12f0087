// arp_poses_fingerprints.h — interaction fingerprints of ligand poses, scored on the device.
//
// The poses result (arp_poses.h) is resident: every pose's ligand - receptor records in ascending (pose, i, j), pose_off, pos_of.
// What a docking or screening run wants of them is small: which poses reproduce the interactions of a few reference poses, which
// receptor nodes the poses touch and how often, and — for a modest number of poses — which poses resemble each other.  A feature
// is (node, plane): the receptor atom (or its residue) of a participating record and one of the 15 SIFt bits.  The first Q poses
// of the launch are the references.  Only ids, count [P], cross [P][Q] and occupancy [U][NP] cross PCIe.
//
// Shape:
//   k_pfp_mark       a thread per record: the node of a participating record sets its bit of a presence bitmap of ceil(N / 64)
//                    words — one relaxed no-return 64-bit OR, skipped when the bit is seen set (pfp_set_bit).  Nodes are dense
//                    small integers: no sort finds the columns.
//   k_pfp_scan       one block: popcount per word, exclusive scan -> base[word], U.  The host waits for U (it sizes the matrix).
//   k_pfp_ids        ids[base[w] + rank of the bit] = 64 w + bit: the columns, ascending.
//   k_pfp_bits       a wave per pose (pose_off gives its records: no search), 64 records a step: column = base[word] +
//                    popcount(presence[word] & bits below); one relaxed no-return OR per plane into the pose's own row of the
//                    zeroed matrix.  The layout is arp_similarity.h's: bits[p][plane][word], plane-major.
//   k_pfp_cross      cross = B R^T by popcount, the rectangular sibling of k_sim_gram: a block owns 64 poses x the (up to 64)
//                    references and a slice of the words, stages both panels in LDS (word-major, 66 words a row: the layout and
//                    the bank argument of arp_similarity.h), a 4 x 4 sub-tile of __popcll(x & y) a thread.  count[p] is the
//                    popcount of the words as they are staged.  One slice: plain stores; several: uint32 atomicAdd into zeroed
//                    arrays (exact in any order).
//   k_pfp_occupancy  column sums of the finished matrix over the poses p >= Q: a block stages 64 poses x 32 words, a wave takes
//                    8 word columns, lane l = pose l reads one word, and 64 ballots transpose it: lane b keeps the count of bit
//                    b.  One uint32 atomicAdd per (block, feature) into the zeroed table at the end.
// The all-pairs matrix is k_sim_gram itself (arp_similarity.h), launched unchanged on this matrix.
// The ring / amide records of the same poses (arp_poses_planes.h) enter the same matrix as 14 further planes through the three
// kernels in the middle of this file; the kernels above and below them run unchanged over the wider plane axis.
// No float exists here; every result is a presence or a count, and an OR / an integer add commute: record order cannot show.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define POSEFP_PLANES 15         // ARP_POSEFP_PLANES: the SIFt bits
#define POSEFP_BY_RESIDUE 1u     // ARP_POSEFP_BY_RESIDUE
#define POSEFP_ALL_PAIRS 2u      // ARP_POSEFP_ALL_PAIRS
#define POSEFP_MAX_REFS 64       // ARP_POSEFP_MAX_REFS: one tile of k_pfp_cross
#define POSEFP_CTYPES 7
#define POSEFP_TILE 64           // poses a tile
#define POSEFP_KC 32             // words of a panel staged at once
#define POSEFP_STRIDE (POSEFP_TILE + 2)
#define POSEFP_SCAN_THREADS 1024

struct PoseFpArgs {
    // the poses result: columns of the sorted slab, offsets per pose, position of an atom in the movable set (-1: receptor)
    const int* ci;
    const int* cj;
    const uint16_t* sift;
    const uint8_t* ctype;
    const unsigned long long* pose_off;      // [P + 1]
    const int* pos_of;                       // [n]
    const int* res_id;                       // [n] (residue level)
    long long k;                             // records
    int P, Q;                                // poses; the first Q are the references
    long long N;                             // nodes: atoms or residues
    int by_res;
    uint32_t planes, ctype_mask;
    // columns
    unsigned long long* presence;            // [NW]
    uint32_t* base;                          // [NW]
    long long NW;
    long long* total;                        // U
    int* ids;                                // [U]
    long long U;
    // bits[p][plane][w]: plane the compact index of a selected plane, w < wpp = ceil(U / 64); W = NP * wpp words a pose
    unsigned long long* bits;
    long long wpp, W;
    int NP;
    // k_pfp_cross: slice y takes the words [y * per, min(W, (y + 1) * per)); per is a multiple of POSEFP_KC
    long long per;
    int slices;
    uint32_t* count;                         // [P]
    uint32_t* cross;                         // [P][Q]
    // k_pfp_occupancy: slice y takes the pose tiles [y * occ_tiles, (y + 1) * occ_tiles)
    uint32_t* occ;                           // [U][NP]
    int occ_tiles;
};

// Set `bit` of *word unless it is seen set already.  Bits are only ever set while a kernel runs, so a set bit that is seen is
// set; a stale read costs one OR too many, never a lost one.  The read keeps the ORs of the many records that share a node (a
// residue has several atoms, a popular node occurs in most poses) from queueing up on one address.
__device__ __forceinline__ void pfp_set_bit(unsigned long long* word, unsigned long long bit) {
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) return;
    (void)__hip_atomic_fetch_or(word, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The two steps of a bits kernel (k_pfp_bits, k_pfp_bits_planes, and k_lfp_bits of arp_library_fingerprints.h):
// the column of a node whose presence bit is set: the set bits in front of it
__device__ __forceinline__ long long pfp_column(const PoseFpArgs& A, long long node) {
    return (long long)A.base[node >> 6] + __popcll(A.presence[node >> 6] & ((1ull << (node & 63)) - 1ull));
}
// column `col` of every plane of m into `row`: plane b of the launch is the compact plane popcount(planes below b)
__device__ __forceinline__ void pfp_or_planes(const PoseFpArgs& A, unsigned long long* row, long long col, uint32_t m) {
    const unsigned long long bit = 1ull << (col & 63);
    unsigned long long* const mine = row + (col >> 6);
    while (m) {
        const int b = __ffs((int)m) - 1;
        m &= m - 1u;
        const long long q = (long long)__popc(A.planes & ((1u << b) - 1u));
        pfp_set_bit(mine + q * A.wpp, bit);
    }
}

// does record r take part, and with which planes
__device__ __forceinline__ uint32_t pfp_record_planes(const PoseFpArgs& A, long long r) {
    const uint32_t ct = A.ctype[r];
    if (ct >= POSEFP_CTYPES || !((A.ctype_mask >> ct) & 1u)) return 0u;
    return (uint32_t)A.sift[r] & A.planes;
}
// the receptor partner of record r: whichever of i / j is not movable; -1 when it is no node (never for a record of the launch)
__device__ __forceinline__ long long pfp_node(const PoseFpArgs& A, long long r) {
    const int i = A.ci[r], j = A.cj[r];
    const int a = A.pos_of[i] < 0 ? i : j;
    const long long node = A.by_res ? (long long)A.res_id[a] : (long long)a;
    return (node >= 0 && node < A.N) ? node : -1;
}

__global__ __launch_bounds__(256) void k_pfp_mark(PoseFpArgs A) {
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < A.k; r += (long long)gridDim.x * blockDim.x) {
        if (!pfp_record_planes(A, r)) continue;
        const long long node = pfp_node(A, r);
        if (node < 0) continue;
        pfp_set_bit(A.presence + (node >> 6), 1ull << (node & 63));
    }
}

// one block: thread t owns a run of consecutive words
__global__ __launch_bounds__(POSEFP_SCAN_THREADS) void k_pfp_scan(PoseFpArgs A) {
    __shared__ uint32_t s_sum[POSEFP_SCAN_THREADS];
    const int t = threadIdx.x;
    const long long per = (A.NW + POSEFP_SCAN_THREADS - 1) / POSEFP_SCAN_THREADS;
    const long long lo = min(A.NW, (long long)t * per), hi = min(A.NW, lo + per);
    uint32_t mine = 0;
    for (long long w = lo; w < hi; ++w) mine += (uint32_t)__popcll(A.presence[w]);
    s_sum[t] = mine;
    __syncthreads();
    for (int d = 1; d < POSEFP_SCAN_THREADS; d <<= 1) {
        const uint32_t v = t >= d ? s_sum[t - d] : 0u;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    uint32_t run = s_sum[t] - mine;
    for (long long w = lo; w < hi; ++w) {
        A.base[w] = run;
        run += (uint32_t)__popcll(A.presence[w]);
    }
    if (t == POSEFP_SCAN_THREADS - 1) *A.total = (long long)s_sum[t];
}

__global__ __launch_bounds__(256) void k_pfp_ids(PoseFpArgs A) {
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < A.NW; w += (long long)gridDim.x * blockDim.x) {
        unsigned long long m = A.presence[w];
        long long o = A.base[w];
        while (m) {
            const int b = __ffsll((unsigned long long)m) - 1;
            m &= m - 1ull;
            if (o < A.U) A.ids[o] = (int)(w * 64 + b);
            ++o;
        }
    }
}

__global__ __launch_bounds__(256) void k_pfp_bits(PoseFpArgs A) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long p = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < A.P; p += waves) {
        const long long s = (long long)A.pose_off[p], e = min((long long)A.pose_off[p + 1], A.k);
        unsigned long long* const row = A.bits + p * A.W;
        for (long long r = s + lane; r < e; r += 64) {
            uint32_t m = pfp_record_planes(A, r);
            if (!m) continue;
            const long long node = pfp_node(A, r);
            if (node < 0) continue;
            const long long col = pfp_column(A, node);
            if (col >= A.U) continue;      // (never: k_pfp_mark set this node's bit)
            pfp_or_planes(A, row, col, m);
        }
    }
}

// ---- the ring / amide classes as planes: the four tables of the poses-planes result (arp_poses_planes.h), which
// is resident beside the poses result and sorted by pose as well.  An entity is on the LIGAND side when it is a movable atom
// (pos_of >= 0), a ring with a movable atom in its path (ring_static == 1) or a moved amide (am_pos >= 0); a ring that a pose
// merely comes near (ring_static 0 or 2) is the receptor's.  A record takes part when bit ctype of ctype_mask is set, exactly
// one of its two entities is on the ligand side and its plane is selected; its node is the residue of the receptor entity.
//   plane 15 + b   atom_plane, bit b of its mask, the ATOM is the ligand's    node: the ring's residue
//   plane 20 + b   atom_plane, bit b of its mask, the RING is the ligand's    node: res_id[atom]
//   plane 25       plane_plane (any class)                                    node: the other ring's residue
//   plane 26       group_group                                                node: am_res of the other amide
//   plane 27       group_plane, the AMIDE is the ligand's                     node: the ring's residue
//   plane 28       group_plane, the RING is the ligand's                      node: am_res[amide]
// The residue of a receptor ring is res_id of the first atom of its path — static, nothing per pose.  It is NOT the posed
// ring_res ("the nearest atom within 3 A of the centre"): a ligand atom that sits on the ring takes that over, and the feature
// would name the ligand's own residue.
//   k_pfp_same_poses   both results keep their uploaded poses: compared as 32-bit words, a mismatch ORs 1 into a flag word
//   k_pfp_mark_planes  grid (x, 4), a row per table: the sibling of k_pfp_mark, into the same presence bitmap, before k_pfp_scan
//   k_pfp_bits_planes  a wave per pose walks the pose's slice of each table (its pose_off): the sibling of k_pfp_bits, into
//                      the same rows, after it.  Kept apart from k_pfp_bits: that kernel stays as 5q measured it, and an
//                      empty table or a pose without records costs two loads of its offsets here.
#define POSEFP_ALL_PLANES 29     // ARP_POSEFP_ALL_PLANES
#define POSEFP_AP_BITS 5         // ARP_AP_CARBONPI ... ARP_AP_METSULPHURPI
#define POSEFP_PLANE_AP_ATOM 15
#define POSEFP_PLANE_AP_RING 20
#define POSEFP_PLANE_PP 25
#define POSEFP_PLANE_GG 26
#define POSEFP_PLANE_GP_AMIDE 27
#define POSEFP_PLANE_GP_RING 28

struct PoseFpTables {
    const int* first[4];                     // atom, bgn, bgn, amide
    const int* second[4];                    // ring, end, end, ring
    const uint8_t* ctype[4];
    const uint8_t* ap_mask;                  // atom_plane: ARP_AP_* bits
    const unsigned long long* pose_off;      // [4][P + 1]
    long long count[4];
    const int* pos_of;                       // [n]: the poses-planes result's
    const uint8_t* ring_static;              // [nring]
    const int* am_pos;                       // [namide]
    const int* ring_off;
    const int* ring_idx;
    const int* am_res;                       // [namide]
    int n, nring, namide;
};

__device__ __forceinline__ int pfp_ring_res(const PoseFpArgs& A, const PoseFpTables& T, int r) {
    const int s = T.ring_off[r];
    return s < T.ring_off[r + 1] ? A.res_id[T.ring_idx[s]] : -1;
}

// the selected planes of record r of table t and its node (-1: none); 0 when the record takes no part.  The table is a template
// parameter: an index into the argument's arrays that is known only at run time would send them to scratch memory
template <int t>
__device__ __forceinline__ uint32_t pfp_class_planes(const PoseFpArgs& A, const PoseFpTables& T, long long r, long long* node) {
    const uint32_t ct = T.ctype[t][r];
    if (ct >= POSEFP_CTYPES || !((A.ctype_mask >> ct) & 1u)) return 0u;
    const int a = T.first[t][r], b = T.second[t][r];
    const int na = t == 0 ? T.n : t == 1 ? T.nring : T.namide, nb = (t == 0 || t == 1 || t == 3) ? T.nring : T.namide;
    if (a < 0 || a >= na || b < 0 || b >= nb) return 0u;      // (never: the ids are those k_poses_planes wrote)
    bool la, lb;
    uint32_t m;
    if (t == 0) {
        la = T.pos_of[a] >= 0; lb = T.ring_static[b] == 1;
        m = ((uint32_t)T.ap_mask[r] & ((1u << POSEFP_AP_BITS) - 1u)) << (la ? POSEFP_PLANE_AP_ATOM : POSEFP_PLANE_AP_RING);
    } else if (t == 1) {
        la = T.ring_static[a] == 1; lb = T.ring_static[b] == 1;
        m = 1u << POSEFP_PLANE_PP;
    } else if (t == 2) {
        la = T.am_pos[a] >= 0; lb = T.am_pos[b] >= 0;
        m = 1u << POSEFP_PLANE_GG;
    } else {
        la = T.am_pos[a] >= 0; lb = T.ring_static[b] == 1;
        m = 1u << (la ? POSEFP_PLANE_GP_AMIDE : POSEFP_PLANE_GP_RING);
    }
    m &= A.planes;
    if (la == lb || !m) return 0u;
    int res;
    if (t == 0) res = la ? pfp_ring_res(A, T, b) : A.res_id[a];
    else if (t == 1) res = pfp_ring_res(A, T, la ? b : a);
    else if (t == 2) res = T.am_res[la ? b : a];
    else res = la ? pfp_ring_res(A, T, b) : T.am_res[a];
    *node = (res >= 0 && (long long)res < A.N) ? (long long)res : -1;
    return m;
}

__global__ __launch_bounds__(256) void k_pfp_same_poses(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, long long words,
                                                        uint32_t* __restrict__ flag) {
    uint32_t differ = 0;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (long long)gridDim.x * blockDim.x) differ |= a[w] ^ b[w];
    if (differ) atomicOr(flag, 1u);
}

template <int t>
__device__ __forceinline__ void pfp_mark_table(const PoseFpArgs& A, const PoseFpTables& T) {
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < T.count[t]; r += (long long)gridDim.x * blockDim.x) {
        long long node = -1;
        if (!pfp_class_planes<t>(A, T, r, &node) || node < 0) continue;
        pfp_set_bit(A.presence + (node >> 6), 1ull << (node & 63));
    }
}
// grid (x, 4): row y marks table y
__global__ __launch_bounds__(256) void k_pfp_mark_planes(PoseFpArgs A, PoseFpTables T) {
    switch (blockIdx.y) {
        case 0: pfp_mark_table<0>(A, T); break;
        case 1: pfp_mark_table<1>(A, T); break;
        case 2: pfp_mark_table<2>(A, T); break;
        default: pfp_mark_table<3>(A, T); break;
    }
}

// the slice of table t that belongs to pose p, 64 records a step, into the pose's row
template <int t>
__device__ __forceinline__ void pfp_bits_table(const PoseFpArgs& A, const PoseFpTables& T, long long p, int lane, unsigned long long* row) {
    if (T.count[t] == 0) return;
    const unsigned long long* const off = T.pose_off + (long long)t * ((long long)A.P + 1) + p;
    const long long s = (long long)off[0], e = min((long long)off[1], T.count[t]);
    for (long long r = s + lane; r < e; r += 64) {
        long long node = -1;
        uint32_t m = pfp_class_planes<t>(A, T, r, &node);
        if (!m || node < 0) continue;
        const long long col = pfp_column(A, node);
        if (col >= A.U) continue;      // (never: k_pfp_mark_planes set this node's bit)
        pfp_or_planes(A, row, col, m);
    }
}
__global__ __launch_bounds__(256) void k_pfp_bits_planes(PoseFpArgs A, PoseFpTables T) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long p = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < A.P; p += waves) {
        unsigned long long* const row = A.bits + p * A.W;
        pfp_bits_table<0>(A, T, p, lane, row);
        pfp_bits_table<1>(A, T, p, lane, row);
        pfp_bits_table<2>(A, T, p, lane, row);
        pfp_bits_table<3>(A, T, p, lane, row);
    }
}

// LDS slot of model m of a tile: arp_similarity.h's, so that a thread's 4 x 4 sub-tile is contiguous in the result
__device__ __forceinline__ int pfp_slot(int m) { return ((m >> 1) & 1) * 32 + (m >> 2) * 2 + (m & 1); }

// grid (pose tiles, slices); four blocks a CU, as k_sim_gram runs: 128 registers a lane
__global__ __launch_bounds__(256, 4) void k_pfp_cross(PoseFpArgs A) {
    __shared__ __attribute__((aligned(16))) unsigned long long s_a[POSEFP_KC * POSEFP_STRIDE];
    __shared__ __attribute__((aligned(16))) unsigned long long s_b[POSEFP_KC * POSEFP_STRIDE];
    constexpr int ROUNDS = POSEFP_TILE * POSEFP_KC / 256;      // staging rounds: a thread stages word k of the poses m0 + 8 it
    static_assert(POSEFP_KC == 32 && ROUNDS == 8, "a staging round is 8 poses x 32 words: the 32 lanes of a half wave share a pose");
    const long long p0 = (long long)blockIdx.x * POSEFP_TILE;
    const long long w_lo = (long long)blockIdx.y * A.per, w_hi = min(A.W, w_lo + A.per);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int k = threadIdx.x & (POSEFP_KC - 1), m0 = threadIdx.x >> 5;
    const bool refs = A.Q > 0;
    uint32_t acc[4][4] = {};
    uint32_t cnt[ROUNDS] = {};
    for (long long w0 = w_lo; w0 < w_hi; w0 += POSEFP_KC) {      // (block-uniform trip count)
        // ---- stage: poses beyond P, references beyond Q and words beyond the slice are zero
        const long long w = w0 + k;
#pragma unroll
        for (int it = 0; it < ROUNDS; ++it) {
            const int m = m0 + 8 * it;
            const long long p = p0 + m;
            const int at = k * POSEFP_STRIDE + pfp_slot(m);
            const unsigned long long x = (p < (long long)A.P && w < w_hi) ? A.bits[p * A.W + w] : 0ull;
            cnt[it] += (uint32_t)__popcll(x);
            s_a[at] = x;
            if (refs) s_b[at] = (m < A.Q && w < w_hi) ? A.bits[(long long)m * A.W + w] : 0ull;
        }
        __syncthreads();
        if (refs) {
#pragma unroll 4
            for (int kk = 0; kk < POSEFP_KC; ++kk) {
                const ulonglong2 a01 = *(const ulonglong2*)&s_a[kk * POSEFP_STRIDE + 2 * ty];
                const ulonglong2 a23 = *(const ulonglong2*)&s_a[kk * POSEFP_STRIDE + 32 + 2 * ty];
                const ulonglong2 b01 = *(const ulonglong2*)&s_b[kk * POSEFP_STRIDE + 2 * tx];
                const ulonglong2 b23 = *(const ulonglong2*)&s_b[kk * POSEFP_STRIDE + 32 + 2 * tx];
                const unsigned long long a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] += (uint32_t)__popcll(a[i] & b[j]);
            }
        }
        __syncthreads();
    }
    const bool add = A.slices > 1;
    // ---- count: the 32 lanes that staged the words of one pose add up (xor distances below 32 stay inside the half wave)
#pragma unroll
    for (int it = 0; it < ROUNDS; ++it) {
        uint32_t v = cnt[it];
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
        const long long p = p0 + m0 + 8 * it;
        if (k == 0 && p < (long long)A.P) {
            if (add) atomicAdd(A.count + p, v);
            else A.count[p] = v;
        }
    }
    if (!refs) return;
    // ---- cross: the thread's sub-tile is poses 4 ty + i, references 4 tx + j
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long p = p0 + 4 * ty + i;
        if (p >= (long long)A.P) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = 4 * tx + j;
            if (q >= A.Q) continue;
            uint32_t* const pq = A.cross + p * (long long)A.Q + q;
            if (add) atomicAdd(pq, acc[i][j]);
            else *pq = acc[i][j];
        }
    }
}

// grid (chunks of POSEFP_KC words, pose slices)
__global__ __launch_bounds__(256) void k_pfp_occupancy(PoseFpArgs A) {
    __shared__ unsigned long long s_x[POSEFP_KC * POSEFP_STRIDE];      // [word][pose]: a wave reads 64 consecutive words
    constexpr int COLS = POSEFP_KC / 4;                                 // word columns a wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w0 = (long long)blockIdx.x * POSEFP_KC;
    const long long tiles = ((long long)A.P + POSEFP_TILE - 1) / POSEFP_TILE;
    const long long t_lo = (long long)blockIdx.y * A.occ_tiles, t_hi = min(tiles, t_lo + A.occ_tiles);
    uint32_t cnt[COLS] = {};
    for (long long t = t_lo; t < t_hi; ++t) {      // (block-uniform trip count)
        for (int idx = threadIdx.x; idx < POSEFP_TILE * POSEFP_KC; idx += 256) {
            const int m = idx / POSEFP_KC, k = idx % POSEFP_KC;
            const long long p = t * POSEFP_TILE + m, w = w0 + k;
            s_x[k * POSEFP_STRIDE + m] = (p >= (long long)A.Q && p < (long long)A.P && w < A.W) ? A.bits[p * A.W + w] : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < COLS; ++c) {
            const unsigned long long x = s_x[(wave * COLS + c) * POSEFP_STRIDE + lane];
            uint32_t got = 0;
#pragma unroll 8
            for (int b = 0; b < 64; ++b) {      // (eight ballots in flight: all 64 at once would spill scalar registers)
                const unsigned long long votes = __ballot(((x >> b) & 1ull) != 0ull);
                got = lane == b ? (uint32_t)__popcll(votes) : got;
            }
            cnt[c] += got;
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
        const long long w = w0 + wave * COLS + c;
        if (w >= A.W) continue;
        const long long plane = w / A.wpp, u = (w % A.wpp) * 64 + lane;
        if (u < A.U && cnt[c]) atomicAdd(A.occ + u * A.NP + plane, cnt[c]);
    }
}
