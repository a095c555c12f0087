// arp_library_shortlist.h — the shortlist of the resident library results: global poses, or ligands by their best pose, ranked on
// the device, only the chosen poses' records compacted for the fetch.
//
// The library result (arp_library.h), the library-planes result (arp_library_planes.h) and the library fingerprint
// (arp_library_fingerprints.h) are resident and sorted by global pose, as the three pose results are sorted by pose; their
// per-pose offsets and summary rows are laid out alike (the planes offsets with the row stride T + 1, T <= 2^20 poses).  So
// the lengths, the offsets and the gather are those of the pose shortlist, unchanged: PslArgs names the library's arrays, P is
// T, and k_psl_lengths / k_psl_offsets / k_psl_gather (arp_poses_shortlist.h) run as they are.  Nothing of the three results is
// written here.
//
// New here:
//   k_lsl_score     the key psl_key(score) and the payload (global pose) per candidate, for the same stable 64-bit sort.
//                   Unit poses: a thread per global pose t — k_psl_score's arithmetic with the fingerprint's row Q + t.
//                   Unit ligands: a wave per ligand over its pose range, a segmented arg-max.  A lane scores its poses
//                   t = first + lane, + 64, ... on the fly in ascending order and keeps the pair (score, pose) of the first
//                   highest; a butterfly over the 64 lanes joins the pairs lexicographically (higher score, then lower pose).
//                   No atomics, no per-ligand table in between.  A ligand without poses gets the key all-ones: scores stay
//                   below 2^61 in magnitude, so no real key is all-ones and those ligands sort behind every candidate; the host
//                   knows how many there are (the launch's pose_off) and never looks that far.
//   k_lsl_ligands   ligand[r] = lig_of[pose of candidate r].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_poses_shortlist.h"

#define LSL_POSES 0         // ARP_LIBRARY_SHORTLIST_POSES
#define LSL_LIGANDS 1       // ARP_LIBRARY_SHORTLIST_LIGANDS

struct LslScore {
    int L, T;
    const long long* lig_pose_off;           // [L + 1] the global poses of ligand l (LibraryResult::tab)
    const uint32_t* summary;                 // [T][16]
    const uint32_t* pl_summary;              // [T][16], nullptr when the planes result is not read
    int w[2 * PSL_SLOTS];
    const uint32_t* fp_count;                // [Q + T]
    const uint32_t* fp_cross;                // [Q + T][Q]
    int Q, ref;
    unsigned long long* key;                 // [T] or [L]
    unsigned long long* val;
};

// the int64 score of global pose t (KIND PSL_SUMMARY or PSL_TANIMOTO), as 5s defines it
template <int KIND>
__device__ __forceinline__ long long lsl_pose_score(const LslScore& A, long long t) {
    if (KIND == PSL_SUMMARY) {
        long long score = 0;
        const uint4* const row = (const uint4*)(A.summary + t * PSL_SLOTS);
#pragma unroll
        for (int q = 0; q < PSL_SLOTS / 4; ++q) {
            const uint4 v = row[q];
            score += (long long)A.w[4 * q] * (long long)v.x + (long long)A.w[4 * q + 1] * (long long)v.y +
                     (long long)A.w[4 * q + 2] * (long long)v.z + (long long)A.w[4 * q + 3] * (long long)v.w;
        }
        if (A.pl_summary) {
            const uint4* const prow = (const uint4*)(A.pl_summary + t * PSL_SLOTS);
#pragma unroll
            for (int q = 0; q < PSL_SLOTS / 4; ++q) {
                const uint4 v = prow[q];
                score += (long long)A.w[PSL_SLOTS + 4 * q] * (long long)v.x + (long long)A.w[PSL_SLOTS + 4 * q + 1] * (long long)v.y +
                         (long long)A.w[PSL_SLOTS + 4 * q + 2] * (long long)v.z + (long long)A.w[PSL_SLOTS + 4 * q + 3] * (long long)v.w;
            }
        }
        return score;
    }
    const long long row = (long long)A.Q + t;      // (the references are the first Q rows, and never candidates)
    const uint32_t mine = A.fp_count[row];
    unsigned long long best = 0;
    const int q_lo = A.ref < 0 ? 0 : A.ref, q_hi = A.ref < 0 ? A.Q : A.ref + 1;
    for (int q = q_lo; q < q_hi; ++q) {
        const unsigned long long s = psl_tanimoto(A.fp_cross[row * A.Q + q], mine, A.fp_count[q]);
        best = s > best ? s : best;
    }
    return (long long)best;
}

// (an instance per unit and kind: one kernel of both kinds holds the 32 weights in scalar registers beside everything else and
// spills 85 of them into vector lanes)
template <int UNIT, int KIND>
__global__ __launch_bounds__(256) void k_lsl_score(LslScore A) {
    if (UNIT == LSL_POSES) {
        for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < A.T; t += (long long)gridDim.x * blockDim.x) {
            A.key[t] = psl_key(lsl_pose_score<KIND>(A, t));
            A.val[t] = (unsigned long long)t;
        }
        return;
    }
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwave = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long l = wave; l < A.L; l += nwave) {
        long long p0 = A.lig_pose_off[l], p1 = A.lig_pose_off[l + 1];
        if (p0 < 0) p0 = 0;                  // (never: the launch checked the ranges)
        if (p1 > A.T) p1 = A.T;
        long long bs = 0;
        int bi = -1;
        for (long long t = p0 + lane; t < p1; t += 64) {
            const long long sc = lsl_pose_score<KIND>(A, t);
            if (bi < 0 || sc > bs) { bs = sc; bi = (int)t; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const long long os = __shfl_xor(bs, o);
            const int oi = __shfl_xor(bi, o);
            if (oi >= 0 && (bi < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; }
        }
        if (lane == 0) {
            A.key[l] = bi < 0 ? ~0ull : psl_key(bs);
            A.val[l] = bi < 0 ? 0ull : (unsigned long long)bi;
        }
    }
}

// ligand[r] of candidate r (psl_candidate: the sorted payloads, or the caller's list)
__global__ __launch_bounds__(256) void k_lsl_ligands(PslArgs A, const int* __restrict__ lig_of, int* __restrict__ ligand) {
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < A.ncand; r += (long long)gridDim.x * blockDim.x) {
        int p;
        long long score;
        psl_candidate(A, (int)r, &p, &score);
        ligand[r] = (p >= 0 && p < A.P) ? lig_of[p] : -1;      // (out of range never: k_psl_lengths raises the error word for it)
    }
}
