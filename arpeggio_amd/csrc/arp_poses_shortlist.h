// arp_poses_shortlist.h — the shortlist of the resident poses result: poses ranked on the device, only the chosen ones' records
// compacted for the fetch.
//
// The poses result (arp_poses.h), the poses-planes result (arp_poses_planes.h) and the fingerprint result
// (arp_poses_fingerprints.h) are resident and sorted by pose; a caller who wants the records of the best hundred of 16 384 poses
// has no use for the other 16 284 poses' records.  Nothing of the three results is written here: every kernel reads them and
// writes the shortlist's own buffers.
//
// Shape:
//   k_psl_score     a thread per ranked pose p >= skip: its int64 score (weighted summary slots, or the Tanimoto similarity to a
//                   reference in 32 fractional bits) as the key ~(score ^ 2^63) — ascending key = descending score — with the
//                   payload p, ascending.  The stable 64-bit sort that follows keeps ties in ascending pose.
//   k_psl_lengths   grid (x, 5), a wave per (candidate r, table t): the candidates are the first min(k, P - skip) poses of the
//                   sorted order (or the caller's list); a candidate below min_score has length 0 in every table — the scores
//                   are sorted, so those are a suffix.  Nothing filtered: the difference of the source's pose_off; filtered:
//                   64 records a step, counted by ballot / popcount.  Row 0 also writes pose, score and the two summary rows.
//   k_psl_offsets   block t: exclusive prefix of table t's lengths with a running carry (scan_round, arp_runs.h) -> off[t][.],
//                   the total into the word block; block 0 counts the kept candidates: K.
//   k_psl_gather    grid (x, 5), a wave per (chosen pose r, table t): the pose's segment of the source, 64 records a step, to
//                   off[t][r] onwards; filtered: the position is the running count plus the ballot's prefix, so the order inside
//                   the pose is the source's.  No atomic decides a position.  Lane l reads record s + l of every column: each
//                   column is one coalesced stream in and, where nothing is dropped, out.
// A pose's segment goes to one wave: a pose holds at most a few thousand records (S atoms with a handful of partners each), a
// shortlist of a hundred is a hundred waves a table, and a full-length shortlist is the plain copy at a wave per pose.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_poses_planes.h"

#define PSL_LIST 0          // ARP_SHORTLIST_LIST
#define PSL_SUMMARY 1       // ARP_SHORTLIST_SUMMARY
#define PSL_TANIMOTO 2      // ARP_SHORTLIST_TANIMOTO
#define PSL_TABLES 5        // atom-atom, then the four tables of the poses-planes result
#define PSL_SLOTS 16        // a summary row of either result
#define PSL_MAX_WEIGHT (1 << 24)
#define PSL_CTYPES_ALL 0x7Fu
#define PSL_E_RANGE 1       // the device's error word: a record would have gone past its table's total

// words[8] of the launch's one wait: K, the five totals, the same-poses flag, the error word
#define PSL_W_K 0
#define PSL_W_TOTAL 1
#define PSL_W_DIFFER 6
#define PSL_W_ERR 7

struct PslArgs {
    // ---- the sources
    const int* ci;
    const int* cj;
    const float* cd;
    const uint16_t* cs;
    const uint8_t* cct;
    const unsigned long long* aa_off;        // [P + 1]
    long long aa_count;
    PplColumns pl;                           // the poses-planes result's columns (tables bits 1 ... 4)
    const unsigned long long* pl_off;        // [4][P + 1]
    long long pl_count[4];
    const uint32_t* summary;                 // [P][16]
    const uint32_t* pl_summary;              // [P][16], nullptr when the planes result is not read
    int P;
    // ---- score
    int kind, skip, M;                       // M = P - skip ranked poses
    int w[2 * PSL_SLOTS];
    const uint32_t* fp_count;                // [P]
    const uint32_t* fp_cross;                // [P][Q]
    int Q, ref;
    unsigned long long* key;
    unsigned long long* val;
    // ---- the candidates: sorted keys and payloads (or the caller's ids), the threshold, the filter
    const unsigned long long* skey;
    const unsigned long long* sval;
    const int* ids;
    int ncand;
    long long min_score;
    uint32_t tables, sift_mask, ctype_mask;
    // ---- the result
    int* pose;                               // [ncand]
    long long* score;                        // [ncand]
    uint32_t* out_summary;                   // [ncand][16]
    uint32_t* out_pl_summary;                // [ncand][16]
    unsigned long long* len;                 // [5][ncand]
    unsigned long long* off;                 // [5][ncand + 1]
    unsigned long long* words;               // [8]
    int* oi;
    int* oj;
    float* od;
    uint16_t* os;
    uint8_t* oct;
    PplColumns opl;
    long long total[PSL_TABLES];             // the lengths' totals as the host read them: no record is written at or beyond
};

__device__ __forceinline__ unsigned long long psl_key(long long score) { return ~((unsigned long long)score ^ (1ull << 63)); }
__device__ __forceinline__ long long psl_score_of(unsigned long long key) { return (long long)(~key ^ (1ull << 63)); }

// floor(t 2^32 / u) for u = |A| + |B| - t, 2^32 for 0 / 0: the similarity in 32 fractional bits
__device__ __forceinline__ unsigned long long psl_tanimoto(uint32_t t, uint32_t a, uint32_t b) {
    const unsigned long long u = (unsigned long long)a + (unsigned long long)b - (unsigned long long)t;
    return u == 0ull ? (1ull << 32) : ((unsigned long long)t << 32) / u;
}

__global__ __launch_bounds__(256) void k_psl_score(PslArgs A) {
    for (long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x; m < A.M; m += (long long)gridDim.x * blockDim.x) {
        const long long p = m + A.skip;
        long long score = 0;
        if (A.kind == PSL_SUMMARY) {
            const uint4* const row = (const uint4*)(A.summary + p * PSL_SLOTS);
#pragma unroll
            for (int q = 0; q < PSL_SLOTS / 4; ++q) {
                const uint4 v = row[q];
                score += (long long)A.w[4 * q] * (long long)v.x + (long long)A.w[4 * q + 1] * (long long)v.y +
                         (long long)A.w[4 * q + 2] * (long long)v.z + (long long)A.w[4 * q + 3] * (long long)v.w;
            }
            if (A.pl_summary) {
                const uint4* const prow = (const uint4*)(A.pl_summary + p * PSL_SLOTS);
#pragma unroll
                for (int q = 0; q < PSL_SLOTS / 4; ++q) {
                    const uint4 v = prow[q];
                    score += (long long)A.w[PSL_SLOTS + 4 * q] * (long long)v.x + (long long)A.w[PSL_SLOTS + 4 * q + 1] * (long long)v.y +
                             (long long)A.w[PSL_SLOTS + 4 * q + 2] * (long long)v.z + (long long)A.w[PSL_SLOTS + 4 * q + 3] * (long long)v.w;
                }
            }
        } else {      // PSL_TANIMOTO
            const uint32_t mine = A.fp_count[p];
            unsigned long long best = 0;
            const int q_lo = A.ref < 0 ? 0 : A.ref, q_hi = A.ref < 0 ? A.Q : A.ref + 1;
            for (int q = q_lo; q < q_hi; ++q) {
                const unsigned long long s = psl_tanimoto(A.fp_cross[p * A.Q + q], mine, A.fp_count[q]);
                best = s > best ? s : best;
            }
            score = (long long)best;
        }
        A.key[m] = psl_key(score);
        A.val[m] = (unsigned long long)p;
    }
}

// candidate r: its pose and score; kept = the score reaches the threshold (a list has no threshold)
__device__ __forceinline__ bool psl_candidate(const PslArgs& A, int r, int* pose, long long* score) {
    if (A.kind == PSL_LIST) {
        *pose = A.ids[r];
        *score = 0;
        return true;
    }
    *pose = (int)A.sval[r];
    *score = psl_score_of(A.skey[r]);
    return *score >= A.min_score;
}

__device__ __forceinline__ bool psl_keep_aa(const PslArgs& A, long long q) {
    const uint32_t ct = A.cct[q];
    if (ct >= 32u || !((A.ctype_mask >> ct) & 1u)) return false;
    return A.sift_mask == 0u || ((uint32_t)A.cs[q] & A.sift_mask) != 0u;
}
// the byte column of table t that holds ctype (arp_poses_planes_fetch's order)
template <int t>
__device__ __forceinline__ bool psl_keep_pl(const PslArgs& A, long long q) {
    const uint32_t ct = A.pl.u[t][t == 0 ? 1 : t == 1 ? 2 : 0][q];
    return ct < 32u && ((A.ctype_mask >> ct) & 1u);
}

// the segment of pose p in table t (0: atom-atom), clamped to the table
template <int t>
__device__ __forceinline__ void psl_segment(const PslArgs& A, int p, long long* s, long long* e) {
    if (t == 0) {
        *s = (long long)A.aa_off[p];
        *e = min((long long)A.aa_off[p + 1], A.aa_count);
    } else {
        const unsigned long long* const off = A.pl_off + (long long)(t - 1) * ((long long)A.P + 1) + p;
        *s = (long long)off[0];
        *e = min((long long)off[1], A.pl_count[t - 1]);
    }
    if (*e < *s) *e = *s;
}

template <int t>
__device__ __forceinline__ void psl_lengths_table(const PslArgs& A, int lane) {
    const bool wanted = (A.tables >> t) & 1u;
    const bool all = t == 0 ? (A.sift_mask == 0u && A.ctype_mask == PSL_CTYPES_ALL) : A.ctype_mask == PSL_CTYPES_ALL;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < A.ncand; r += waves) {
        int p;
        long long score;
        bool kept = psl_candidate(A, (int)r, &p, &score);
        if (p < 0 || p >= A.P) {      // (never: the host checked a list's ids, the payloads are those k_psl_score wrote)
            if (lane == 0) A.words[PSL_W_ERR] = PSL_E_RANGE;
            p = 0;
            kept = false;
        }
        if (t == 0) {      // the per-pose arrays ride in row 0
            if (lane == 0) { A.pose[r] = p; A.score[r] = score; }
            if (lane < PSL_SLOTS) A.out_summary[r * PSL_SLOTS + lane] = A.summary[(long long)p * PSL_SLOTS + lane];
            else if (lane < 2 * PSL_SLOTS && A.pl_summary) A.out_pl_summary[r * PSL_SLOTS + lane - PSL_SLOTS] = A.pl_summary[(long long)p * PSL_SLOTS + lane - PSL_SLOTS];
        }
        long long n = 0;
        if (wanted && kept) {      // (wave-uniform)
            long long s, e;
            psl_segment<t>(A, p, &s, &e);
            if (all) n = e - s;
            else
                for (long long q0 = s; q0 < e; q0 += 64) {
                    const long long q = q0 + lane;
                    const bool keep = q < e && (t == 0 ? psl_keep_aa(A, q) : psl_keep_pl<t == 0 ? 0 : t - 1>(A, q));
                    n += (long long)__popcll(__ballot(keep));
                }
        }
        if (lane == 0) A.len[(long long)t * A.ncand + r] = (unsigned long long)n;
    }
}
// grid (x, 5): row y is table y
__global__ __launch_bounds__(256) void k_psl_lengths(PslArgs A) {
    const int lane = threadIdx.x & 63;
    switch (blockIdx.y) {
        case 0: psl_lengths_table<0>(A, lane); break;
        case 1: psl_lengths_table<1>(A, lane); break;
        case 2: psl_lengths_table<2>(A, lane); break;
        case 3: psl_lengths_table<3>(A, lane); break;
        default: psl_lengths_table<4>(A, lane); break;
    }
}

// block t: off[t][r] = kept records of table t in the candidates before r, off[t][ncand] = all of them (a candidate below the
// threshold has length 0: off[t][K] is the total as well).  Block 0 counts the candidates that are kept.
__global__ __launch_bounds__(1024) void k_psl_offsets(PslArgs A) {
    __shared__ unsigned long long s_w[16];
    __shared__ unsigned int s_kept;
    const int t = (int)blockIdx.x;
    const unsigned long long* const len = A.len + (long long)t * A.ncand;
    unsigned long long* const out = A.off + (long long)t * ((long long)A.ncand + 1);
    if (threadIdx.x == 0) s_kept = 0u;
    unsigned long long carry = 0;
    unsigned int kept = 0;
    for (int r0 = 0; r0 < A.ncand; r0 += 1024) {
        const int r = r0 + (int)threadIdx.x;
        const unsigned long long v = r < A.ncand ? len[r] : 0ull;
        if (t == 0 && r < A.ncand) {
            int p;
            long long score;
            kept += psl_candidate(A, r, &p, &score) ? 1u : 0u;
        }
        const unsigned long long before = scan_round(v, s_w, carry);
        if (r < A.ncand) out[r] = before;
    }
    if (threadIdx.x == 0) {
        out[A.ncand] = carry;
        A.words[PSL_W_TOTAL + t] = carry;
    }
    if (t == 0) {
        __syncthreads();
        if (kept) atomicAdd(&s_kept, kept);
        __syncthreads();
        if (threadIdx.x == 0) A.words[PSL_W_K] = (unsigned long long)s_kept;
    }
}

// record q of table t to place `to` of the shortlist's columns
template <int t>
__device__ __forceinline__ void psl_copy(const PslArgs& A, long long q, long long to) {
    if (t == 0) {
        A.oi[to] = A.ci[q]; A.oj[to] = A.cj[q]; A.od[to] = A.cd[q]; A.os[to] = A.cs[q]; A.oct[to] = A.cct[q];
        return;
    }
    constexpr int b = t == 0 ? 0 : t - 1;
    A.opl.i0[b][to] = A.pl.i0[b][q];
    A.opl.i1[b][to] = A.pl.i1[b][q];
    if (b == 2) {      // group-group: float32 behind the same pointers
#pragma unroll
        for (int c = 0; c < 3; ++c) ((float*)A.opl.d[2][c])[to] = ((const float*)A.pl.d[2][c])[q];
    } else {
        constexpr int nv = b == 0 ? 2 : b == 1 ? 4 : 3;
#pragma unroll
        for (int c = 0; c < nv; ++c) A.opl.d[b][c][to] = A.pl.d[b][c][q];
    }
    constexpr int nu = b == 0 ? 2 : b == 1 ? 3 : 1;
#pragma unroll
    for (int c = 0; c < nu; ++c) A.opl.u[b][c][to] = A.pl.u[b][c][q];
}

template <int t>
__device__ __forceinline__ void psl_gather_table(const PslArgs& A, int lane) {
    if (!((A.tables >> t) & 1u) || A.total[t] == 0) return;
    const bool all = t == 0 ? (A.sift_mask == 0u && A.ctype_mask == PSL_CTYPES_ALL) : A.ctype_mask == PSL_CTYPES_ALL;
    const unsigned long long* const off = A.off + (long long)t * ((long long)A.ncand + 1);
    const unsigned long long lt = (1ull << lane) - 1ull;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    bool past = false;
    for (long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < A.ncand; r += waves) {
        long long at = (long long)off[r];
        const long long end = (long long)off[r + 1];
        if (end <= at) continue;      // (nothing kept of this pose: also every candidate below the threshold)
        long long s, e;
        psl_segment<t>(A, A.pose[r], &s, &e);
        for (long long q0 = s; q0 < e; q0 += 64) {
            const long long q = q0 + lane;
            const bool keep = q < e && (all || (t == 0 ? psl_keep_aa(A, q) : psl_keep_pl<t == 0 ? 0 : t - 1>(A, q)));
            const unsigned long long votes = __ballot(keep);
            const long long to = at + (long long)__popcll(votes & lt);
            if (keep) {
                if (to < end && to < A.total[t]) psl_copy<t>(A, q, to);
                else past = true;
            }
            at += (long long)__popcll(votes);
        }
    }
    if (past) A.words[PSL_W_ERR] = PSL_E_RANGE;      // (never: the lengths were counted with the same predicate)
}
// grid (x, 5): row y is table y
__global__ __launch_bounds__(256) void k_psl_gather(PslArgs A) {
    const int lane = threadIdx.x & 63;
    switch (blockIdx.y) {
        case 0: psl_gather_table<0>(A, lane); break;
        case 1: psl_gather_table<1>(A, lane); break;
        case 2: psl_gather_table<2>(A, lane); break;
        case 3: psl_gather_table<3>(A, lane); break;
        default: psl_gather_table<4>(A, lane); break;
    }
}
