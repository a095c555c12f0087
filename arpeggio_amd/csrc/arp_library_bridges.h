// arp_library_bridges.h — ligand-water-receptor contacts of every pose of the resident library result: the
// library's records (t, i, a) joined on the device with the atom-atom bag of a pass over the receptor alone, everything selected.
// A RECEPTOR LEG is arp_bridge.h's leg of that bag: a record with exactly one water atom w and a wanted SIFt bit, partner j.  A
// LIGAND LEG of pose t is a library record (t, i, a) with ARP_F_WATER on receptor atom i = w, none on library atom a and a wanted
// bit.  One row (t, w, a, j) per ligand leg and receptor leg of the same water, ascending by (t, w, a, j): the ligand legs arrive
// in that order, a water's receptor legs are sorted by partner, and the rank of a row is its global index — nothing sorts the
// output.  No atomics on global memory, no look-back, no block waits for another, plain stores:
//   (k_bridge_legs_count / k_runs_scan / k_bridge_legs_write, the key sort and k_runs_count / _scan / _starts of arp_bridge.h over
//   the receptor's bag, unchanged: L_r sorted legs — wait 1 — and the starts of their U runs)
//   k_libbridge_table   run r -> water_legs[w] = (first leg, legs): a table by atom id, zero-filled before, so that a ligand leg
//                       finds its water's receptor legs with one load; U goes beside the totals below
//   k_libbridge_count   block b, the tiling of k_filter_count: ligand legs, rows (64-bit) and (pose, water) heads of tile b
//   k_libbridge_scan    one block: exclusive prefixes of the three in place; totals = ligand legs, rows B, heads
//   (the host reads the totals — wait 2, the last — and sizes the eight columns)
//   k_libbridge_write   block b: the tile's ligand legs staged in LDS with their exclusive row prefixes; each lane takes
//                       consecutive rows, finds its leg by binary search there, its receptor leg at first + (row - prefix), and
//                       writes row tile prefix + row of all eight columns; the three prefixes at every pose's first record -> at
//   k_libbridge_poses   pose t: bridge_off[t] = rows before its first record, waters[t] and legs[t] from the same prefixes
// A HEAD is a ligand leg whose water has a receptor leg and that no earlier ligand leg of the same pose shares its water with:
// the records of one (pose, water) are consecutive and at most one per ligand atom, so the walk back is short.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_bridge.h"

struct LibBridgeArgs {
    // the library result's records, sorted by (t, i, a), and its poses
    const int* ri;
    const int* ra;
    const float* rd;
    const uint16_t* rs;
    long long k;                        // records
    const unsigned long long* pose_off; // [T + 1], pose_off[T] = k
    int T;
    const int* lig_of;                  // [T]
    const int* atom_off;                // [ligands + 1]
    const uint16_t* rec_flags;          // per receptor atom
    const uint16_t* lib_flags;          // per library atom
    int n;                              // receptor atoms
    uint32_t sift_any;                  // low 15 bits
    // the receptor's legs, sorted by (w, partner), and where each water's begin
    const unsigned long long* lkey;
    const unsigned long long* lval;
    long long rlegs;                    // L_r
    int pbits;
    const int* row_start;               // [U] (made for L_r runs: row_start[U] is NOT the end of the last)
    const long long* runs;              // [1]: U
    uint2* water_legs;                  // [n]: (first leg, legs) of water w, (0, 0) without one
    // counts
    long long* tile;                    // [3 tiles]: ligand legs | rows | heads of every tile, then their exclusive prefixes
    int tiles;
    long long* totals;                  // [4]: ligand legs, rows, heads, U
    long long* at;                      // [3 T]: the three prefixes at the first record of every pose that has one
    long long rows;                     // B
    // the table, one column after the other
    int* t_pose;
    int* t_water;
    int* t_lig;
    int* t_rec;
    float* t_dl;
    float* t_dr;
    uint16_t* t_sl;
    uint16_t* t_sr;
    // per pose
    unsigned long long* bridge_off;     // [T + 1]
    uint32_t* waters;                   // [T]
    uint32_t* legs;                     // [T]
};

// the pose of record rr < k: the last t with pose_off[t] <= rr (pose_off[0] = 0, pose_off[T] = k)
__device__ __forceinline__ int libbridge_pose_of(const LibBridgeArgs& A, long long rr) {
    int lo = 0, hi = A.T;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)A.pose_off[mid] <= rr) lo = mid; else hi = mid;
    }
    return lo;
}

// record rr of pose t with a wanted bit and a water i: is library atom a no water?
__device__ __forceinline__ bool libbridge_ligand_side(const LibBridgeArgs& A, int t, long long rr) {
    return (A.lib_flags[A.atom_off[A.lig_of[t]] + A.ra[rr]] & BRIDGE_F_WATER) == 0;
}

// Bit r of the result: record lo + r of the thread's FILTER_ITEMS consecutive records is a ligand leg; then t[r] is its pose and
// wl[r] its water's (first receptor leg, receptor legs).  *heads: the legs among them that are heads.  The SIFt test comes first
// (one 16-byte load where the eight are all there): atoms, flags and pose are read for the records that pass it only.
__device__ __forceinline__ uint32_t libbridge_legs(const LibBridgeArgs& A, long long lo, int t[FILTER_ITEMS], uint2 wl[FILTER_ITEMS], uint32_t* heads) {
    static_assert(FILTER_ITEMS == 8, "one uint4 of SIFt words per thread");
    *heads = 0u;
#pragma unroll
    for (int r = 0; r < FILTER_ITEMS; ++r) { t[r] = 0; wl[r] = make_uint2(0u, 0u); }
    if (lo >= A.k) return 0u;
    uint32_t sf[FILTER_ITEMS];
    if (lo + FILTER_ITEMS <= A.k && (((uintptr_t)(A.rs + lo)) & 15) == 0) {
        const uint4 s4 = *reinterpret_cast<const uint4*>(A.rs + lo);
        const uint32_t sw[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int r = 0; r < FILTER_ITEMS; ++r) sf[r] = (sw[r >> 1] >> (16 * (r & 1))) & 0xFFFFu;
    } else {
#pragma unroll
        for (int r = 0; r < FILTER_ITEMS; ++r) sf[r] = lo + r < A.k ? (uint32_t)A.rs[lo + r] : 0u;
    }
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < FILTER_ITEMS; ++r) {
        if ((sf[r] & A.sift_any) == 0u) continue;
        const long long rr = lo + r;
        const int i = A.ri[rr];
        if ((uint32_t)i >= (uint32_t)A.n || (A.rec_flags[i] & BRIDGE_F_WATER) == 0) continue;
        const int tt = libbridge_pose_of(A, rr);
        if (!libbridge_ligand_side(A, tt, rr)) continue;
        m |= 1u << r;
        t[r] = tt;
        wl[r] = A.water_legs[i];
        if (wl[r].y == 0u) continue;
        bool head = true;
        for (long long q = rr - 1; q >= (long long)A.pose_off[tt] && A.ri[q] == i; --q)
            if ((A.rs[q] & A.sift_any) != 0u && libbridge_ligand_side(A, tt, q)) { head = false; break; }
        *heads |= (head ? 1u : 0u) << r;
    }
    return m;
}

__global__ __launch_bounds__(256) void k_libbridge_table(LibBridgeArgs A) {
    const long long U = min(A.runs[0], A.rlegs);
    if (blockIdx.x == 0 && threadIdx.x == 0) A.totals[3] = U;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < U; r += (long long)gridDim.x * blockDim.x) {
        const long long s = A.row_start[r], e = r + 1 < U ? (long long)A.row_start[r + 1] : A.rlegs;
        if (s < 0 || s >= A.rlegs || e <= s) continue;
        const unsigned long long w = A.lkey[s] >> A.pbits;
        if (w < (unsigned long long)A.n) A.water_legs[w] = make_uint2((uint32_t)s, (uint32_t)(e - s));
    }
}

__global__ __launch_bounds__(FILTER_THREADS) void k_libbridge_count(LibBridgeArgs A) {
    __shared__ long long s_w[SORT_WAVES];
    static_assert(FILTER_THREADS == SORT_THREADS, "sort_block_scan scans SORT_THREADS values");
    int t[FILTER_ITEMS];
    uint2 wl[FILTER_ITEMS];
    uint32_t heads;
    const uint32_t m = libbridge_legs(A, (long long)blockIdx.x * FILTER_TILE + (long long)threadIdx.x * FILTER_ITEMS, t, wl, &heads);
    long long nr = 0;
#pragma unroll
    for (int r = 0; r < FILTER_ITEMS; ++r) nr += (long long)wl[r].y;
    long long tl, tr, th;
    (void)sort_block_scan((long long)__popc(m), s_w, &tl);
    (void)sort_block_scan(nr, s_w, &tr);
    (void)sort_block_scan((long long)__popc(heads), s_w, &th);
    if (threadIdx.x == 0) {
        A.tile[blockIdx.x] = tl;
        A.tile[(size_t)A.tiles + blockIdx.x] = tr;
        A.tile[2 * (size_t)A.tiles + blockIdx.x] = th;
    }
}

// one block (SORT_THREADS threads: sort_block_scan): exclusive 64-bit prefix of each of the three per-tile counts in place, their
// sums to totals[0 ... 2]
__global__ __launch_bounds__(SORT_THREADS) void k_libbridge_scan(LibBridgeArgs A) {
    __shared__ long long s_w[SORT_WAVES];
    for (int q = 0; q < 3; ++q) {
        long long* const v = A.tile + (size_t)q * A.tiles;
        long long run = 0;
        for (int t0 = 0; t0 < A.tiles; t0 += SORT_THREADS) {      // (block-uniform trip count)
            const int t = t0 + threadIdx.x;
            const long long x = t < A.tiles ? v[t] : 0;
            long long sum;
            const long long e = sort_block_scan(x, s_w, &sum);
            if (t < A.tiles) v[t] = run + e;
            run += sum;
        }
        if (threadIdx.x == 0) A.totals[q] = run;
    }
}

__global__ __launch_bounds__(FILTER_THREADS) void k_libbridge_write(LibBridgeArgs A) {
    __shared__ long long s_w[SORT_WAVES];
    __shared__ long long s_pre[FILTER_TILE + 1];      // exclusive row prefix of the tile's ligand leg q, inside the tile
    __shared__ int s_first[FILTER_TILE];              // its water's first receptor leg
    __shared__ int s_t[FILTER_TILE];                  // its pose
    __shared__ unsigned short s_rec[FILTER_TILE];     // its record, inside the tile
    const long long tile_lo = (long long)blockIdx.x * FILTER_TILE;
    const long long lo = tile_lo + (long long)threadIdx.x * FILTER_ITEMS;
    int t[FILTER_ITEMS];
    uint2 wl[FILTER_ITEMS];
    uint32_t heads;
    const uint32_t m = libbridge_legs(A, lo, t, wl, &heads);
    long long nr = 0;
#pragma unroll
    for (int r = 0; r < FILTER_ITEMS; ++r) nr += (long long)wl[r].y;
    long long tl, tr;
    const long long legs_x = sort_block_scan((long long)__popc(m), s_w, &tl);
    const long long rows_x = sort_block_scan(nr, s_w, &tr);
    const long long heads_x = sort_block_scan((long long)__popc(heads), s_w, nullptr);
    const long long gl = A.tile[blockIdx.x], gr = A.tile[(size_t)A.tiles + blockIdx.x], gh = A.tile[2 * (size_t)A.tiles + blockIdx.x];
    // ---- the ligand legs of the tile, staged; the prefixes at every pose's first record
    {
        int q = (int)legs_x;
        long long pre = rows_x, nh = heads_x;
        int tc = -1;
        long long next = 0;      // first record of pose tc + 1
#pragma unroll
        for (int r = 0; r < FILTER_ITEMS; ++r) {
            const long long rr = lo + r;
            if (rr < A.k) {
                if (tc < 0 || rr >= next) { tc = libbridge_pose_of(A, rr); next = (long long)A.pose_off[tc + 1]; }
                if ((long long)A.pose_off[tc] == rr) {
                    A.at[tc] = gl + q;
                    A.at[(size_t)A.T + tc] = gr + pre;
                    A.at[2 * (size_t)A.T + tc] = gh + nh;
                }
            }
            if ((m >> r) & 1u) {
                if (q < FILTER_TILE) {      // (q < the tile's legs <= FILTER_TILE always)
                    s_pre[q] = pre; s_first[q] = (int)wl[r].x; s_t[q] = t[r]; s_rec[q] = (unsigned short)(threadIdx.x * FILTER_ITEMS + r);
                }
                ++q;
                pre += (long long)wl[r].y;
                nh += (heads >> r) & 1u;
            }
        }
    }
    if (threadIdx.x == 0) s_pre[tl] = tr;
    __syncthreads();
    // ---- the rows of the tile: consecutive lanes, consecutive rows
    const unsigned long long pmask = (1ull << A.pbits) - 1ull;
    for (long long row = threadIdx.x; row < tr; row += FILTER_THREADS) {
        int a = 0, b = (int)tl;      // s_pre[a] <= row < s_pre[b]
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (s_pre[mid] <= row) a = mid; else b = mid;
        }
        const long long p = (long long)s_first[a] + (row - s_pre[a]);
        const long long g = gr + row;
        if (p < A.rlegs && g < A.rows) {      // (always: B is the sum of the same counts, a run lies inside the legs)
            const long long rr = tile_lo + s_rec[a];
            const unsigned long long key = A.lkey[p], val = A.lval[p];
            A.t_pose[g] = s_t[a];
            A.t_water[g] = (int)(key >> A.pbits);
            A.t_lig[g] = A.ra[rr];
            A.t_rec[g] = (int)(key & pmask);
            A.t_dl[g] = A.rd[rr];
            A.t_dr[g] = payload_distance(val);
            A.t_sl[g] = A.rs[rr];
            A.t_sr[g] = (uint16_t)payload_sift(val);
        }
    }
}

// thread t <= T: the prefixes at the first record at or behind pose t's begin — those of the pose that owns that record, or the
// totals behind the last record
__global__ __launch_bounds__(256) void k_libbridge_poses(LibBridgeArgs A) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > A.T) return;
    long long p[2][3];
    for (int e = 0; e < 2; ++e) {
        const long long u = min(t + e, (long long)A.T);
        const long long rr = (long long)A.pose_off[u];
        if (rr >= A.k) { for (int q = 0; q < 3; ++q) p[e][q] = A.totals[q]; }
        else { const int v = libbridge_pose_of(A, rr); for (int q = 0; q < 3; ++q) p[e][q] = A.at[(size_t)q * A.T + v]; }
    }
    A.bridge_off[t] = (unsigned long long)p[0][1];
    if (t < A.T) {
        A.legs[t] = (uint32_t)(p[1][0] - p[0][0]);
        A.waters[t] = (uint32_t)(p[1][2] - p[0][2]);
    }
}
