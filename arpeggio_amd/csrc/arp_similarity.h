// arp_similarity.h — interaction-fingerprint similarity between the models of an ensemble, made on the device.
//
// The persistence tables say in how many models a contact exists; this says which models share their contacts: inter[f][g] =
// features present in model f AND in model g, a feature being (row, plane) — a row of the persistence table (atom level) or of
// the residue persistence table (residue level), a plane one of the 15 SIFt bits or one of the five record classes.  The
// result is F x F uint32 whatever the structure size, so only it crosses PCIe.
//
// Shape: the re-key, the radix passes and the run kernels of the table it shares its rows with, unchanged, and then
//   k_sim_bits   one wave per row, 64 consecutive sorted records per step (the loop of k_persist_reduce): record -> model f
//                (low fbits of the key) and the planes it has; one relaxed 64-bit OR per plane into bits[f][plane][row >> 6].
//                An OR is idempotent and commutes: several records of one (row, model) and the order of the records cannot show.
//   k_sim_gram   inter = B B^T by popcount: a block owns a 64 x 64 tile of model pairs (tf <= tg) and a slice of the words,
//                stages both 64-model panels of SIM_KC words in LDS, and every thread adds __popcll(x & y) into a 4 x 4
//                sub-tile.  One slice: plain stores; several: integer atomicAdd into the zeroed matrix (exact in any order).
// No float exists here.
//
// LDS panels (MI355X: 64 banks of 4 B; ds_read_b128 is serviced in groups of 16 lanes, ds_write_b64 banks by (a / 4) mod 32):
// word-major, s[w][slot], SIM_STRIDE = 66 words a row.  A thread's four models of a panel are the slots {2 t, 2 t + 1} and
// {32 + 2 t, 33 + 2 t} (t = its 0 ... 15 coordinate), i.e. two 16-byte reads per panel and word.  The 16 lanes of a read group
// then cover 16 consecutive 16-byte pieces = 64 distinct banks (column panel), or two adjacent pieces broadcast (row panel):
// no conflict.  Slot s holds model 4 (s / 2 % 16) + 2 (s / 32) + s % 2 of the tile, so that a thread's 4 x 4 sub-tile is
// CONTIGUOUS in the matrix (rows 4 ty ... 4 ty + 3, columns 4 tx ... 4 tx + 3).  The staging writes walk the words of one model
// with consecutive lanes (coalesced global reads); their stride of 66 words = 132 dwords puts the 16 lanes of a write group on
// banks 0, 4, ... 60 mod 32: two-way, which a 64-bit store absorbs (its data transfer is longer than two array cycles).
// Without the two words of padding it would be 16-way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_runs.h"

#define SIM_PLANES 20            // ARP_SIM_PLANES: 15 SIFt bits, then the five record classes
#define SIM_BY_RESIDUE 1u        // ARP_SIM_BY_RESIDUE
#define SIM_TILE 64              // models a side of a k_sim_gram tile
#define SIM_KC 32                // words of a panel staged at once: 2 x 32 x 66 x 8 B = 33 KiB of LDS
#define SIM_STRIDE (SIM_TILE + 2)

struct SimArgs {
    // the re-keyed records, sorted (model = key & fmask), and their rows
    const unsigned long long* key;
    const unsigned long long* val;
    const int* row_start;    // [U + 1] (RunArgs)
    long long U;
    int fbits;
    uint32_t planes, ctype_mask;
    uint32_t F;              // resident models
    // bits[f][p][w]: p the compact index of a selected plane, w < wpp = ceil(U / 64); W = popcount(planes) * wpp words a model
    unsigned long long* bits;
    long long wpp, W;
    // k_sim_gram: slice y of the grid takes the words [y * per, min(W, (y + 1) * per)); per is a multiple of SIM_KC
    long long per;
    int slices, tiles;       // tiles = ceil(F / SIM_TILE) a side
    uint32_t* inter;         // [F][F]
};

// the planes a record has: an admitted atom-atom record its SIFt bits and plane 15, a ring / amide record plane 15 + class
__device__ __forceinline__ uint32_t sim_record_planes(unsigned long long v, uint32_t ctype_mask) {
    const uint32_t cls = payload_class(v);
    if (cls == 0u) return ((ctype_mask >> payload_type(v)) & 1u) ? (payload_sift(v) | (1u << TABLE_SIFT_BITS)) : 0u;
    return cls <= 4u ? 1u << (TABLE_SIFT_BITS + cls) : 0u;      // (TABLE_LEFT_OUT: none)
}

__global__ __launch_bounds__(256) void k_sim_bits(SimArgs A) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const unsigned long long fmask = (1ull << A.fbits) - 1ull;
    for (long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < A.U; row += waves) {
        // (the last row's range also holds the left-out records that trail it: they have no plane)
        const long long s = A.row_start[row], e = A.row_start[row + 1];
        const unsigned long long bit = 1ull << (row & 63);
        const long long w = row >> 6;
        for (long long q = s + lane; q < e; q += 64) {
            uint32_t m = sim_record_planes(A.val[q], A.ctype_mask) & A.planes;
            const uint32_t f = (uint32_t)(A.key[q] & fmask);
            if (f >= A.F) continue;      // (never for a kept record: the re-key wrote f < F)
            unsigned long long* const mine = A.bits + (long long)f * A.W + w;
            while (m) {
                const int b = __ffs((int)m) - 1;
                m &= m - 1u;
                const long long p = (long long)__popc(A.planes & ((1u << b) - 1u));
                __hip_atomic_fetch_or(mine + p * A.wpp, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// model of the tile that LDS slot s holds (see the head of this file); its inverse places a model's words
__device__ __forceinline__ int sim_slot_of_model(int m) { return ((m >> 1) & 1) * 32 + (m >> 2) * 2 + (m & 1); }

// grid (tile pairs tf <= tg, slices)
__global__ __launch_bounds__(256) void k_sim_gram(SimArgs A) {
    __shared__ __attribute__((aligned(16))) unsigned long long s_a[SIM_KC * SIM_STRIDE];
    __shared__ __attribute__((aligned(16))) unsigned long long s_b[SIM_KC * SIM_STRIDE];
    // ---- which tile: pair index -> (tf, tg), row tf of the upper triangle holds tiles - tf pairs
    int tf = 0, rest = (int)blockIdx.x;
    while (rest >= A.tiles - tf) { rest -= A.tiles - tf; ++tf; }      // (block-uniform; at most `tiles` steps)
    const int tg = tf + rest;
    const long long w_lo = (long long)blockIdx.y * A.per, w_hi = min(A.W, w_lo + A.per);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    uint32_t acc[4][4] = {};
    for (long long w0 = w_lo; w0 < w_hi; w0 += SIM_KC) {      // (block-uniform trip count)
        // ---- stage: SIM_TILE models x SIM_KC words of either panel; models beyond F and words beyond the slice are zero
        for (int idx = threadIdx.x; idx < SIM_TILE * SIM_KC; idx += 256) {
            const int m = idx / SIM_KC, k = idx % SIM_KC;
            const long long w = w0 + k;
            const long long f = (long long)tf * SIM_TILE + m, g = (long long)tg * SIM_TILE + m;
            const int at = k * SIM_STRIDE + sim_slot_of_model(m);
            s_a[at] = (f < (long long)A.F && w < w_hi) ? A.bits[f * A.W + w] : 0ull;
            s_b[at] = (g < (long long)A.F && w < w_hi) ? A.bits[g * A.W + w] : 0ull;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < SIM_KC; ++k) {
            const ulonglong2 a01 = *(const ulonglong2*)&s_a[k * SIM_STRIDE + 2 * ty];
            const ulonglong2 a23 = *(const ulonglong2*)&s_a[k * SIM_STRIDE + 32 + 2 * ty];
            const ulonglong2 b01 = *(const ulonglong2*)&s_b[k * SIM_STRIDE + 2 * tx];
            const ulonglong2 b23 = *(const ulonglong2*)&s_b[k * SIM_STRIDE + 32 + 2 * tx];
            const unsigned long long a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += (uint32_t)__popcll(a[i] & b[j]);
        }
        __syncthreads();
    }
    // ---- write: the thread's sub-tile is rows 4 ty + i, columns 4 tx + j of the tile
    const bool diagonal = tf == tg, add = A.slices > 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long f = (long long)tf * SIM_TILE + 4 * ty + i;
        if (f >= (long long)A.F) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long g = (long long)tg * SIM_TILE + 4 * tx + j;
            if (g >= (long long)A.F) continue;
            uint32_t* const fg = A.inter + f * (long long)A.F + g;
            uint32_t* const gf = A.inter + g * (long long)A.F + f;
            if (add) {
                atomicAdd(fg, acc[i][j]);
                if (!diagonal) atomicAdd(gf, acc[i][j]);      // (the diagonal tile computes [g][f] itself)
            } else {
                *fg = acc[i][j];
                if (!diagonal) *gf = acc[i][j];
            }
        }
    }
}
