// arp_coupling.h — contact coupling over the models of an ensemble: which contacts form and break together, correlated on the
// device.
//
// Similarity (arp_similarity.h) is B B^T over models; this is B^T B over contacts.  A row is a contact — a row of the
// persistence table (atom level) or of the residue persistence table (residue level) —, present or absent in each of the F
// models; the rows whose number of models lies in an occupancy band are the K features; and a pair of features u < v with n11
// models in common is kept when phi^2 >= q / 1024, as a comparison of integers:
//     d = F n11 - n_u n_v,    1024 d^2 >= q n_u (F - n_u) n_v (F - n_v).
// With F <= 4096 both sides stay below 2^58 (|d| <= F^2 / 4 = 2^22, n (F - n) <= 2^22).  Only the kept pairs leave the device.
//
// Shape: the re-key, the radix passes and the run kernels of the table it shares its rows with, unchanged, and then
//   k_couple_bits      one wave per row, 64 consecutive sorted records per step: lane L holds word L of the row's model bits
//                      (fw = ceil(F / 64) <= 64 words), OR-reduced over the wave by shuffles — one wave owns a row, so there is
//                      no atomic —; rowbits[row][fw] (feature-major: the transpose of k_sim_bits' layout) and n_row, a popcount.
//   k_couple_keep      the rows of a tile of COUPLE_TILE_ROWS that lie in the band, counted (k_runs_scan: the host learns K)
//   k_couple_compact   the kept rows at their rank: their bits packed, n, and the feature table (a, b, count)
//   k_couple_gram      n11 = B^T B by popcount: a block owns a 64 x 64 tile of feature pairs (tu <= tv), stages both panels in
//                      LDS in the layout arp_similarity.h documents (word-major, stride SIM_STRIDE, sim_slot_of_model), and
//                      every thread adds __popcll(x & y) into a 4 x 4 sub-tile over ALL fw words — the criterion needs the
//                      complete sum, so there are no word slices; the tile pairs supply the parallelism.  The epilogue
//                      evaluates the criterion in registers and appends the kept pairs, one atomic add of the running total
//                      per wave that keeps any: key = u << vbits | v, value = n11.  Nothing is written at or beyond `cap`,
//                      and the total counts every kept pair, so it is exact on overflow.
//   (the radix passes of arp_sort.h over the 2 vbits key bits: ascending (u, v), whatever order the waves appended in)
//   k_couple_rows      the sorted pairs into the columns u, v, n11
// No float exists here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_similarity.h"

#define COUPLE_BY_RESIDUE 1u           // ARP_COUPLE_BY_RESIDUE
#define COUPLE_MAX_FEATURES 65536      // ARP_COUPLE_MAX_FEATURES
#define COUPLE_MAX_WORDS 64            // fw for ARP_SIM_MAX_MODELS: a word a lane
#define COUPLE_TILE_ROWS 256           // rows a block of k_couple_keep / k_couple_compact

struct CoupleArgs {
    // the re-keyed records, sorted (model = key & fmask), and their rows
    const unsigned long long* key;
    const unsigned long long* val;
    const int* row_start;    // [U + 1] (RunArgs)
    long long U;
    int fbits, bbits;        // key = id_a << (bbits + fbits) | id_b << fbits | model
    uint32_t planes, ctype_mask;
    uint32_t F;              // resident models
    int fw;                  // ceil(F / 64)
    unsigned long long* rowbits;   // [U][fw]
    uint32_t* n_row;               // [U]
    // the band and the compaction
    uint32_t min_count, max_count;
    int* tile_keep;          // [ceil(U / COUPLE_TILE_ROWS)]: kept rows of the tile, then their exclusive prefix
    long long K;
    unsigned long long* bits;      // [K][fw]: the kept rows' bits
    uint32_t* n;                   // [K]
    int32_t *t_a, *t_b;            // the feature table
    uint32_t* t_count;
    // the product
    int tiles;               // ceil(K / SIM_TILE) a side
    uint32_t q;              // phi2_q
    int vbits;               // bits of a feature index
    unsigned long long* total;     // running total of kept pairs (zeroed)
    unsigned long long* pair_key;  // [cap]
    unsigned long long* pair_val;  // [cap]
    long long cap;
    // the rows of the pair table
    long long P;
    uint32_t *t_u, *t_v, *t_n11;
};

__global__ __launch_bounds__(256) void k_couple_bits(CoupleArgs A) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const unsigned long long fmask = (1ull << A.fbits) - 1ull;
    for (long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < A.U; row += waves) {
        // (the last row's range also holds the left-out records that trail it: they have no plane)
        const long long s = A.row_start[row], e = A.row_start[row + 1];
        unsigned long long mine = 0ull;      // word `lane` of the row
        for (long long q0 = s; q0 < e; q0 += 64) {      // (wave-uniform trip count)
            const long long q = q0 + lane;
            uint32_t f = 0u;
            bool on = false;
            if (q < e) {
                f = (uint32_t)(A.key[q] & fmask);
                on = f < A.F && (sim_record_planes(A.val[q], A.ctype_mask) & A.planes) != 0u;      // (f < F for every kept record)
            }
            // the records of a row ascend by model: the words this step touches lie between its first and its last record's
            const int last = (int)min((long long)63, e - 1 - q0);
            const int w_lo = __shfl((int)(f >> 6), 0), w_hi = min(__shfl((int)(f >> 6), last), A.fw - 1);
            for (int w = w_lo; w <= w_hi; ++w) {      // (wave-uniform)
                unsigned long long x = on && (int)(f >> 6) == w ? 1ull << (f & 63u) : 0ull;
                for (int o = 32; o > 0; o >>= 1) x |= __shfl_xor(x, o);
                if (lane == w) mine |= x;
            }
        }
        if (lane < A.fw) A.rowbits[row * A.fw + lane] = mine;
        int c = __popcll(mine);
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) A.n_row[row] = (uint32_t)c;
    }
}

__device__ __forceinline__ bool couple_kept(const CoupleArgs& A, long long row) {
    if (row >= A.U) return false;
    const uint32_t n = A.n_row[row];
    return n >= A.min_count && n <= A.max_count;
}

// grid: the tiles of COUPLE_TILE_ROWS rows
__global__ __launch_bounds__(COUPLE_TILE_ROWS) void k_couple_keep(CoupleArgs A) {
    __shared__ int s_w[COUPLE_TILE_ROWS / 64];
    int c = couple_kept(A, (long long)blockIdx.x * COUPLE_TILE_ROWS + threadIdx.x) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < COUPLE_TILE_ROWS / 64; ++w) t += s_w[w];
        A.tile_keep[blockIdx.x] = t;
    }
}

// grid: the same tiles, after k_runs_scan made tile_keep the exclusive prefix
__global__ __launch_bounds__(COUPLE_TILE_ROWS) void k_couple_compact(CoupleArgs A) {
    static_assert(COUPLE_TILE_ROWS == SORT_THREADS, "sort_block_scan scans SORT_THREADS values");
    __shared__ long long s_w[SORT_WAVES];
    __shared__ int s_rank[COUPLE_TILE_ROWS];      // rank of the tile's row among the features, or -1
    const long long row0 = (long long)blockIdx.x * COUPLE_TILE_ROWS, row = row0 + threadIdx.x;
    const bool keep = couple_kept(A, row);
    const long long rank = (long long)A.tile_keep[blockIdx.x] + sort_block_scan(keep ? 1ll : 0ll, s_w, nullptr);
    const bool put = keep && rank < A.K;      // (rank < K always: K is the sum of the same counts)
    s_rank[threadIdx.x] = put ? (int)rank : -1;
    if (put) {
        const unsigned long long pair = A.key[A.row_start[row]] >> A.fbits;
        A.t_a[rank] = (int32_t)(pair >> A.bbits);
        A.t_b[rank] = (int32_t)(pair & ((1ull << A.bbits) - 1ull));
        A.t_count[rank] = A.n[rank] = A.n_row[row];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < COUPLE_TILE_ROWS * A.fw; idx += COUPLE_TILE_ROWS) {
        const int r = idx / A.fw, w = idx % A.fw;
        const int at = s_rank[r];
        if (at >= 0) A.bits[(long long)at * A.fw + w] = A.rowbits[(row0 + r) * A.fw + w];
    }
}

// grid: the tile pairs tu <= tv of the upper triangle
__global__ __launch_bounds__(256) void k_couple_gram(CoupleArgs A) {
    __shared__ __attribute__((aligned(16))) unsigned long long s_a[SIM_KC * SIM_STRIDE];
    __shared__ __attribute__((aligned(16))) unsigned long long s_b[SIM_KC * SIM_STRIDE];
    int tu = 0, rest = (int)blockIdx.x;
    while (rest >= A.tiles - tu) { rest -= A.tiles - tu; ++tu; }      // (block-uniform; at most `tiles` steps)
    const int tv = tu + rest;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    uint32_t acc[4][4] = {};
    for (int w0 = 0; w0 < A.fw; w0 += SIM_KC) {      // (block-uniform trip count: at most two panels)
        const int kc = min(SIM_KC, A.fw - w0);
        // ---- stage: SIM_TILE features x kc words of either panel; features beyond K are zero
        for (int idx = threadIdx.x; idx < SIM_TILE * kc; idx += 256) {
            const int m = idx / kc, k = idx % kc;
            const long long u = (long long)tu * SIM_TILE + m, v = (long long)tv * SIM_TILE + m;
            const int at = k * SIM_STRIDE + sim_slot_of_model(m);
            s_a[at] = u < A.K ? A.bits[u * A.fw + w0 + k] : 0ull;
            s_b[at] = v < A.K ? A.bits[v * A.fw + w0 + k] : 0ull;
        }
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
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
    // ---- the criterion: the thread's sub-tile is features 4 ty + i of tile tu against 4 tx + j of tile tv
    const long long F = (long long)A.F;
    const long long u0 = (long long)tu * SIM_TILE + 4 * ty, v0 = (long long)tv * SIM_TILE + 4 * tx;
    long long nu[4], nv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        nu[i] = u0 + i < A.K ? (long long)A.n[u0 + i] : 0ll;
        nv[i] = v0 + i < A.K ? (long long)A.n[v0 + i] : 0ll;
    }
    uint32_t kept = 0u;      // bit 4 i + j
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long u = u0 + i, v = v0 + j;
            const long long d = F * (long long)acc[i][j] - nu[i] * nv[j];
            const unsigned long long lhs = 1024ull * (unsigned long long)(d * d);
            const unsigned long long rhs = (unsigned long long)A.q * (unsigned long long)(nu[i] * (F - nu[i])) * (unsigned long long)(nv[j] * (F - nv[j]));
            if (u < v && v < A.K && lhs >= rhs) kept |= 1u << (4 * i + j);      // (u < v: the diagonal tile's upper half)
        }
    // ---- append: the wave's kept pairs take consecutive slots from the running total
    const int lane = threadIdx.x & 63;
    const int mine = __popc(kept);
    int incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    const int wave_total = __shfl(incl, 63);
    if (wave_total == 0) return;      // (wave-uniform)
    unsigned long long base = 0ull;
    if (lane == 63) base = atomicAdd(A.total, (unsigned long long)wave_total);
    base = __shfl(base, 63);
    long long at = (long long)base + (incl - mine);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((kept >> (4 * i + j)) & 1u) {
                if (at < A.cap) {
                    A.pair_key[at] = (unsigned long long)(u0 + i) << A.vbits | (unsigned long long)(v0 + j);
                    A.pair_val[at] = (unsigned long long)acc[i][j];
                }
                ++at;
            }
}

__global__ __launch_bounds__(256) void k_couple_rows(CoupleArgs A) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const unsigned long long vmask = (1ull << A.vbits) - 1ull;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < A.P; p += stride) {
        const unsigned long long k = A.pair_key[p];
        A.t_u[p] = (uint32_t)(k >> A.vbits);
        A.t_v[p] = (uint32_t)(k & vmask);
        A.t_n11[p] = (uint32_t)A.pair_val[p];
    }
}
